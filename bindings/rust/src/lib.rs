//! Drop-in façade with the reference's API (`DenoiseState`, `RnnModel`, jneem/nnnoiseless src/denoise.rs,
//! src/rnn.rs) over the MI355X backend's C ABI (include/nnn_batch.h).  Written against the FFI only;
//! it was not compiled in the build image, which has no Rust toolchain.
use std::os::raw::{c_float, c_int, c_long, c_void};

#[repr(C)]
pub struct RawModel {
    _p: [u8; 0],
}
#[repr(C)]
pub struct RawBatch {
    _p: [u8; 0],
}
#[repr(C)]
pub struct RawNode {
    _p: [u8; 0],
}
#[repr(C)]
pub struct RawRate {
    _p: [u8; 0],
}
#[repr(C)]
pub struct RawTrain {
    _p: [u8; 0],
}
#[repr(C)]
pub struct RawSim {
    _p: [u8; 0],
}
#[repr(C)]
pub struct RawPack {
    _p: [u8; 0],
}
#[repr(C)]
pub struct RawFit {
    _p: [u8; 0],
}
#[repr(C)]
pub struct RawScore {
    _p: [u8; 0],
}
#[repr(C)]
pub struct RawGate {
    _p: [u8; 0],
}
#[repr(C)]
pub struct RawMix {
    _p: [u8; 0],
}
#[repr(C)]
pub struct RawPick {
    _p: [u8; 0],
}

extern "C" {
    fn nnn_model_from_bytes(bytes: *const u8, len: usize) -> *mut RawModel;
    fn nnn_model_default() -> *mut RawModel;
    fn nnn_model_free(m: *mut RawModel);
    fn nnn_model_clone(m: *const RawModel) -> *mut RawModel;
    fn nnn_node_create(model: *const RawModel, n_streams: c_int, devices: *const c_int, n_devices: c_int, opts: *const BatchOpts) -> *mut RawNode;
    fn nnn_node_destroy(n: *mut RawNode);
    fn nnn_node_reset(n: *mut RawNode) -> c_int;
    fn nnn_node_process_host(
        n: *mut RawNode,
        input: *const c_float,
        output: *mut c_float,
        vad: *mut c_float,
        n_frames: c_int,
        stream_stride: usize,
        frame_stride: usize,
    ) -> c_int;
    fn nnn_node_num_shards(n: *const RawNode) -> c_int;
    fn nnn_node_shard_cpus(n: *const RawNode, i: c_int) -> *const std::os::raw::c_char;
    fn nnn_node_synchronize(n: *mut RawNode) -> c_int;
    fn nnn_node_process_device_streams(
        n: *mut RawNode,
        d_in: *const *const c_float,
        d_out: *const *mut c_float,
        d_vad: *const *mut c_float,
        hip_streams: *const *mut c_void,
        n_tables: c_int,
        n_frames: c_int,
        stream_stride: usize,
        frame_stride: usize,
    ) -> c_int;
    fn nnn_batch_create(model: *const RawModel, n_streams: c_int, device: c_int) -> *mut RawBatch;
    fn nnn_batch_destroy(b: *mut RawBatch);
    fn nnn_batch_reset(b: *mut RawBatch) -> c_int;
    fn nnn_batch_clone(b: *mut RawBatch) -> *mut RawBatch;
    fn nnn_batch_process_host(
        b: *mut RawBatch,
        input: *const c_float,
        output: *mut c_float,
        vad: *mut c_float,
        n_frames: c_int,
        stream_stride: usize,
        frame_stride: usize,
    ) -> c_int;
    fn nnn_batch_process_device(
        b: *mut RawBatch,
        d_in: *const c_float,
        d_out: *mut c_float,
        d_vad: *mut c_float,
        n_frames: c_int,
        stream_stride: usize,
        frame_stride: usize,
        hip_stream: *mut c_void,
    ) -> c_int;
    fn nnn_batch_network_device(
        b: *mut RawBatch,
        d_features: *const c_float,
        d_silence: *const i32,
        d_gains: *mut c_float,
        d_vad: *mut c_float,
        n_frames: c_int,
        hip_stream: *mut c_void,
    ) -> c_int;
    fn nnn_batch_network_host(
        b: *mut RawBatch,
        features: *const c_float,
        silence: *const i32,
        gains: *mut c_float,
        vad: *mut c_float,
        n_frames: c_int,
    ) -> c_int;
    fn nnn_batch_fault(b: *const RawBatch) -> c_int;
    fn nnn_batch_hold_streams(b: *mut RawBatch, streams: *const c_int, n: c_int) -> c_int;
    fn nnn_batch_resume_streams(b: *mut RawBatch, streams: *const c_int, n: c_int) -> c_int;
    fn nnn_batch_num_held(b: *const RawBatch) -> c_int;
    fn nnn_batch_held_mask(b: *const RawBatch, held: *mut u8, n: usize) -> c_int;
    fn nnn_batch_set_gain_floor(b: *mut RawBatch, streams: *const c_int, n: c_int, floors: *const c_float, bands: c_int) -> c_int;
    fn nnn_batch_get_gain_floor(b: *mut RawBatch, streams: *const c_int, n: c_int, floors: *mut c_float) -> c_int;
    fn nnn_batch_num_floored(b: *const RawBatch) -> c_int;
    fn nnn_batch_set_channel_link(b: *mut RawBatch, channels: c_int, mode: c_int) -> c_int;
    fn nnn_batch_get_channel_link(b: *const RawBatch, channels: *mut c_int, mode: *mut c_int) -> c_int;
    fn nnn_host_alloc(bytes: usize) -> *mut c_void;
    fn nnn_host_free(p: *mut c_void);
    fn nnn_model_from_rnnoise_text(text: *const u8, len: usize) -> *mut RawModel;
    fn nnn_batch_create_grouped(
        models: *const *const RawModel,
        group_streams: *const c_int,
        n_groups: c_int,
        device: c_int,
    ) -> *mut RawBatch;
    fn nnn_batch_create_opts(
        models: *const *const RawModel,
        group_streams: *const c_int,
        n_groups: c_int,
        device: c_int,
        opts: *const BatchOpts,
    ) -> *mut RawBatch;
    fn nnn_batch_device_bytes(b: *const RawBatch) -> usize;
    fn nnn_batch_process_pcm_host(
        b: *mut RawBatch,
        input: *const c_void,
        output: *mut c_void,
        vad: *mut c_float,
        n_frames: c_int,
        layout: *const PcmLayout,
    ) -> c_int;
    // include/nnn_rate.h
    fn nnn_rate_create(b: *mut RawBatch, source_rate: f64, max_in: c_long) -> *mut RawRate;
    fn nnn_rate_destroy(a: *mut RawRate);
    fn nnn_rate_reset(a: *mut RawRate) -> c_int;
    fn nnn_rate_reset_streams(a: *mut RawRate, streams: *const c_int, n: c_int) -> c_int;
    fn nnn_rate_max_output(a: *const RawRate, n_in: c_long) -> c_long;
    fn nnn_rate_max_frames(a: *const RawRate, n_in: c_long) -> c_int;
    fn nnn_rate_carried(a: *const RawRate) -> c_long;
    fn nnn_rate_process_device(
        a: *mut RawRate,
        d_in: *const c_void,
        n_in: c_long,
        in_stride: usize,
        d_out: *mut c_void,
        cap_out: c_long,
        out_stride: usize,
        n_out: *mut c_long,
        d_vad: *mut c_float,
        cap_frames: c_int,
        n_frames: *mut c_int,
        format: c_int,
        hip_stream: *mut c_void,
    ) -> c_int;
    fn nnn_rate_process_host(
        a: *mut RawRate,
        input: *const c_void,
        n_in: c_long,
        output: *mut c_void,
        cap_out: c_long,
        n_out: *mut c_long,
        vad: *mut c_float,
        cap_frames: c_int,
        n_frames: *mut c_int,
        format: c_int,
    ) -> c_int;
    // include/nnn_pack.h
    fn nnn_pack_create(b: *mut RawBatch, channels: c_int, step_frames: c_int) -> *mut RawPack;
    fn nnn_pack_destroy(p: *mut RawPack);
    fn nnn_pack_plan(
        n_slots: c_int,
        step_frames: c_int,
        file_frames: *const u64,
        n_files: c_int,
        slot_of_file: *mut i32,
        first_step_of_file: *mut i32,
        summary: *mut i64,
    ) -> c_int;
    fn nnn_pack_run_device(
        p: *mut RawPack,
        d_in: *const c_void,
        in_elems: u64,
        in_format: c_int,
        d_out: *mut c_void,
        out_elems: u64,
        out_format: c_int,
        d_vad: *mut c_float,
        vad_elems: u64,
        files: *const PackFile,
        n_files: c_int,
        hip_stream: *mut c_void,
    ) -> c_int;
    fn nnn_pack_run_host(
        p: *mut RawPack,
        input: *const c_void,
        in_elems: u64,
        in_format: c_int,
        output: *mut c_void,
        out_elems: u64,
        out_format: c_int,
        vad: *mut c_float,
        vad_elems: u64,
        files: *const PackFile,
        n_files: c_int,
    ) -> c_int;
    fn nnn_pack_last_summary(p: *const RawPack, summary: *mut i64) -> c_int;
    // include/nnn_train.h
    fn nnn_train_create(n_streams: c_int, device: c_int) -> *mut RawTrain;
    fn nnn_train_destroy(t: *mut RawTrain);
    fn nnn_train_reset(t: *mut RawTrain) -> c_int;
    fn nnn_train_process_host(
        t: *mut RawTrain,
        signal: *const c_float,
        noise: *const c_float,
        combined: *const c_float,
        cutoff: *const i32,
        vad: *const c_float,
        rows: *mut c_float,
        n_frames: c_int,
    ) -> c_int;
    // include/nnn_sim.h
    fn nnn_sim_create(t: *mut RawTrain) -> *mut RawSim;
    fn nnn_sim_destroy(sim: *mut RawSim);
    fn nnn_sim_load(sim: *mut RawSim, which: c_int, pcm: *const i16, elems: u64) -> c_int;
    fn nnn_sim_adopt_device(sim: *mut RawSim, which: c_int, d_pcm: *const i16, elems: u64) -> c_int;
    fn nnn_sim_set_params(sim: *mut RawSim, streams: *const c_int, n: c_int, recs: *const SimParams) -> c_int;
    fn nnn_sim_get_params(sim: *mut RawSim, streams: *const c_int, n: c_int, recs: *mut SimParams) -> c_int;
    fn nnn_sim_reset(sim: *mut RawSim) -> c_int;
    fn nnn_sim_process_device(sim: *mut RawSim, d_sig_off: *const u64, d_noise_off: *const u64, d_rows: *mut c_float, n_frames: c_int, hip_stream: *mut c_void) -> c_int;
    fn nnn_sim_process_host(sim: *mut RawSim, sig_off: *const u64, noise_off: *const u64, rows: *mut c_float, n_frames: c_int) -> c_int;
    fn nnn_sim_signals_host(
        sim: *mut RawSim,
        sig_off: *const u64,
        noise_off: *const u64,
        signal: *mut c_float,
        noise: *mut c_float,
        combined: *mut c_float,
        cutoff: *mut i32,
        vad: *mut c_float,
        n_frames: c_int,
    ) -> c_int;
    fn nnn_sim_fault(sim: *mut RawSim) -> c_int;
    // include/nnn_fit.h
    fn nnn_fit_create(rnn_bytes: *const u8, len: usize, max_seq: c_int, max_window: c_int, device: c_int) -> *mut RawFit;
    fn nnn_fit_destroy(f: *mut RawFit);
    fn nnn_fit_get(f: *mut RawFit, which: c_int, out: *mut c_float) -> c_int;
    fn nnn_fit_set(f: *mut RawFit, which: c_int, values: *const c_float) -> c_int;
    fn nnn_fit_get_step(f: *mut RawFit, step: *mut i64) -> c_int;
    fn nnn_fit_set_step(f: *mut RawFit, step: i64) -> c_int;
    fn nnn_fit_get_settings(f: *mut RawFit, s: *mut FitSettings) -> c_int;
    fn nnn_fit_set_settings(f: *mut RawFit, s: *const FitSettings) -> c_int;
    fn nnn_fit_export_rnn(f: *mut RawFit, out: *mut u8, cap: usize) -> c_int;
    fn nnn_fit_forward_host(f: *mut RawFit, rows: *const c_float, n_seq: c_int, window: c_int, gains: *mut c_float, vad: *mut c_float) -> c_int;
    fn nnn_fit_loss_host(f: *mut RawFit, rows: *const c_float, w: *const c_float, n_seq: c_int, window: c_int) -> c_int;
    fn nnn_fit_grad_host(f: *mut RawFit, rows: *const c_float, w: *const c_float, n_seq: c_int, window: c_int) -> c_int;
    fn nnn_fit_step(f: *mut RawFit, hip_stream: *mut c_void) -> c_int;
    fn nnn_fit_losses(f: *mut RawFit, out: *mut c_float) -> c_int;
    // include/nnn_score.h
    fn nnn_score_create(n_streams: c_int, max_delay: c_int, device: c_int) -> *mut RawScore;
    fn nnn_score_destroy(h: *mut RawScore);
    fn nnn_score_set_delay(h: *mut RawScore, idx: *const c_int, n: c_int, delays: *const i32) -> c_int;
    fn nnn_score_get_delay(h: *mut RawScore, idx: *const c_int, n: c_int, delays: *mut i32) -> c_int;
    fn nnn_score_reset(h: *mut RawScore, idx: *const c_int, n: c_int) -> c_int;
    fn nnn_score_accumulate_device(
        h: *mut RawScore,
        d_ref: *const c_float,
        d_test: *const c_float,
        d_valid: *const u8,
        d_frame_sums: *mut f64,
        n_frames: c_int,
        stream_stride: usize,
        frame_stride: usize,
        hip_stream: *mut c_void,
    ) -> c_int;
    fn nnn_score_accumulate_host(h: *mut RawScore, reference: *const c_float, test: *const c_float, valid: *const u8, frame_sums: *mut f64, n_frames: c_int) -> c_int;
    fn nnn_score_totals(h: *mut RawScore, out: *mut f64, counts: *mut u64) -> c_int;
    fn nnn_score_totals_device(h: *mut RawScore, d_out: *mut f64, d_counts: *mut u64, hip_stream: *mut c_void) -> c_int;
    // include/nnn_gate.h
    fn nnn_gate_create(n_streams: c_int, max_lookback: c_int, device: c_int) -> *mut RawGate;
    fn nnn_gate_destroy(g: *mut RawGate);
    fn nnn_gate_set_params(g: *mut RawGate, idx: *const c_int, n: c_int, params: *const GateParams) -> c_int;
    fn nnn_gate_get_params(g: *mut RawGate, idx: *const c_int, n: c_int, params: *mut GateParams) -> c_int;
    fn nnn_gate_reset(g: *mut RawGate, idx: *const c_int, n: c_int) -> c_int;
    fn nnn_gate_apply_device(
        g: *mut RawGate,
        d_in: *const c_float,
        d_out: *mut c_float,
        d_vad: *const c_float,
        d_live: *const u8,
        d_open: *mut u8,
        n_frames: c_int,
        stream_stride: usize,
        frame_stride: usize,
        hip_stream: *mut c_void,
    ) -> c_int;
    fn nnn_gate_apply_pcm_device(
        g: *mut RawGate,
        d_in: *const c_void,
        d_out: *mut c_void,
        d_vad: *const c_float,
        d_live: *const u8,
        d_open: *mut u8,
        n_frames: c_int,
        layout: *const PcmLayout,
        hip_stream: *mut c_void,
    ) -> c_int;
    fn nnn_gate_apply_host(g: *mut RawGate, input: *const c_float, out: *mut c_float, vad: *const c_float, live: *const u8, open: *mut u8, n_frames: c_int) -> c_int;
    fn nnn_gate_state_bytes(g: *const RawGate) -> usize;
    fn nnn_gate_export_streams(g: *mut RawGate, idx: *const c_int, n: c_int, records: *mut c_void, bytes: usize) -> c_int;
    fn nnn_gate_import_streams(g: *mut RawGate, idx: *const c_int, n: c_int, records: *const c_void, bytes: usize) -> c_int;
    // include/nnn_mix.h
    fn nnn_mix_create(n_streams: c_int, device: c_int) -> *mut RawMix;
    fn nnn_mix_destroy(m: *mut RawMix);
    fn nnn_mix_set_rooms(m: *mut RawMix, idx: *const c_int, n: c_int, room: *const i32) -> c_int;
    fn nnn_mix_get_rooms(m: *mut RawMix, idx: *const c_int, n: c_int, room: *mut i32) -> c_int;
    fn nnn_mix_set_gains(m: *mut RawMix, idx: *const c_int, n: c_int, gain: *const c_float) -> c_int;
    fn nnn_mix_get_gains(m: *mut RawMix, idx: *const c_int, n: c_int, gain: *mut c_float) -> c_int;
    fn nnn_mix_reset(m: *mut RawMix, idx: *const c_int, n: c_int) -> c_int;
    fn nnn_mix_apply_device(
        m: *mut RawMix,
        d_in: *const c_float,
        d_out: *mut c_float,
        d_talk: *const u8,
        d_live: *const u8,
        d_heard: *mut i32,
        n_frames: c_int,
        in_stream_stride: usize,
        in_frame_stride: usize,
        out_stream_stride: usize,
        out_frame_stride: usize,
        hip_stream: *mut c_void,
    ) -> c_int;
    fn nnn_mix_apply_pcm_device(
        m: *mut RawMix,
        d_in: *const c_void,
        d_out: *mut c_void,
        d_talk: *const u8,
        d_live: *const u8,
        d_heard: *mut i32,
        n_frames: c_int,
        in_layout: *const PcmLayout,
        out_layout: *const PcmLayout,
        hip_stream: *mut c_void,
    ) -> c_int;
    fn nnn_mix_apply_host(m: *mut RawMix, input: *const c_float, out: *mut c_float, talk: *const u8, live: *const u8, heard: *mut i32, n_frames: c_int) -> c_int;
    // include/nnn_pick.h
    fn nnn_pick_create(n_streams: c_int, device: c_int) -> *mut RawPick;
    fn nnn_pick_destroy(p: *mut RawPick);
    fn nnn_pick_set_rooms(p: *mut RawPick, idx: *const c_int, n: c_int, room: *const i32) -> c_int;
    fn nnn_pick_get_rooms(p: *mut RawPick, idx: *const c_int, n: c_int, room: *mut i32) -> c_int;
    fn nnn_pick_set_pinned(p: *mut RawPick, idx: *const c_int, n: c_int, pinned: *const u8) -> c_int;
    fn nnn_pick_get_pinned(p: *mut RawPick, idx: *const c_int, n: c_int, pinned: *mut u8) -> c_int;
    fn nnn_pick_set_policy(p: *mut RawPick, k: c_int, decay: c_float, stick: c_float) -> c_int;
    fn nnn_pick_get_policy(p: *mut RawPick, k: *mut c_int, decay: *mut c_float, stick: *mut c_float) -> c_int;
    fn nnn_pick_reset(p: *mut RawPick, idx: *const c_int, n: c_int) -> c_int;
    fn nnn_pick_select_device(
        p: *mut RawPick,
        d_in: *const c_float,
        d_open: *const u8,
        d_live: *const u8,
        d_talk: *mut u8,
        d_dominant: *mut i32,
        d_level: *mut f64,
        n_frames: c_int,
        stream_stride: usize,
        frame_stride: usize,
        hip_stream: *mut c_void,
    ) -> c_int;
    fn nnn_pick_select_pcm_device(
        p: *mut RawPick,
        d_in: *const c_void,
        d_open: *const u8,
        d_live: *const u8,
        d_talk: *mut u8,
        d_dominant: *mut i32,
        d_level: *mut f64,
        n_frames: c_int,
        layout: *const PcmLayout,
        hip_stream: *mut c_void,
    ) -> c_int;
    fn nnn_pick_select_host(p: *mut RawPick, input: *const c_float, open: *const u8, live: *const u8, talk: *mut u8, dominant: *mut i32, level: *mut f64, n_frames: c_int) -> c_int;
}

/// `struct nnn_gate_params` (include/nnn_gate.h): a stream's gate.  `threshold` and `level` in [0, 1], `grace` 0 ..= 6000 frames,
/// `lookback` 0 ..= the object's `max_lookback` frames.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct GateParams {
    pub threshold: f32,
    pub grace: i32,
    pub lookback: i32,
    pub level: f32,
}

/// `struct nnn_pack_file` (include/nnn_pack.h): where a file lies in the input arena, its length in sample frames (samples per channel),
/// and where its audio and its VAD values go; offsets in elements of the respective arena's format.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PackFile {
    pub in_off: u64,
    pub n_frames_samples: u64,
    pub out_off: u64,
    pub vad_off: u64,
}

/// The packer's input formats beside 0 (f32 in i16 range) and 1 (i16): `enum nnn_pack_format`.
pub const PACK_I24: c_int = 16;
pub const PACK_I32: c_int = 17;
pub const PACK_F32_WAV: c_int = 18;

/// `struct nnn_pcm_layout` (include/nnn_batch.h): the sample formats and channel interleave of the reference's callers
/// (src/nnnoiseless.rs:147-177,301-331, src/signal.rs:95-100,123-127), converted inside the first and last kernels.
#[repr(C)]
pub struct PcmLayout {
    pub format: c_int,        // 0 = f32 in i16 range, 1 = i16, 2 = f32 in [-1, 1]
    pub channels: c_int,
    pub discard_first: c_int, // drop the first frame after new()/reset, as the CLI and DenoiseSignal do
    pub reserved: c_int,
    pub group_stride: usize,  // elements between groups of `channels` interleaved streams
    pub frame_stride: usize,  // elements between frames of a group (>= 480 * channels)
}

/// Model parameters; `from_bytes` returns `None` exactly where the reference does (src/rnn.rs:196-222).
pub struct RnnModel(*mut RawModel);
unsafe impl Send for RnnModel {}
unsafe impl Sync for RnnModel {}

impl RnnModel {
    pub fn from_bytes(bytes: &[u8]) -> Option<RnnModel> {
        let p = unsafe { nnn_model_from_bytes(bytes.as_ptr(), bytes.len()) };
        if p.is_null() {
            None
        } else {
            Some(RnnModel(p))
        }
    }
    pub fn from_static_bytes(bytes: &'static [u8]) -> Option<RnnModel> {
        Self::from_bytes(bytes)
    }
    /// An RNNoise text model (what train/convert_rnnoise.py converts first).
    pub fn from_rnnoise_text(text: &str) -> Option<RnnModel> {
        let p = unsafe { nnn_model_from_rnnoise_text(text.as_ptr(), text.len()) };
        if p.is_null() {
            None
        } else {
            Some(RnnModel(p))
        }
    }
}
impl Default for RnnModel {
    fn default() -> RnnModel {
        RnnModel(unsafe { nnn_model_default() })
    }
}
/// The gain floor of an attenuation limit: "never take a band down by more than `db` dB" = `10^(-db / 20)` (`BatchDenoiser::set_gain_floor`).
pub fn attenuation_limit_db(db: f32) -> f32 {
    10f32.powf(-db / 20.0)
}

/// `enum nnn_link_mode`: how the channels of a link group share one gain per band (`BatchDenoiser::set_channel_link`).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(i32)]
pub enum LinkMode {
    Off = 0,
    /// the largest of the channels' network outputs: a band is kept if any channel's network keeps it
    Max = 1,
    /// the smallest
    Min = 2,
}

/// `#[derive(Clone)]` in the reference (src/rnn.rs:54): an independent copy of the parameters (`nnn_model_clone`).
impl Clone for RnnModel {
    fn clone(&self) -> RnnModel {
        let p = unsafe { nnn_model_clone(self.0 as *const RawModel) };
        assert!(!p.is_null(), "nnnoiseless-mi355x: model clone failed");
        RnnModel(p)
    }
}
impl Drop for RnnModel {
    fn drop(&mut self) {
        unsafe { nnn_model_free(self.0) }
    }
}

/// `n` independent denoisers advanced in lock-step (the loop of src/signal.rs:102-104 as one call).
pub struct BatchDenoiser {
    raw: *mut RawBatch,
    n: usize,
}
unsafe impl Send for BatchDenoiser {}
// The reference asserts `DenoiseState: Send + Sync` (src/denoise.rs:125).  Every call that touches the batch's state takes
// `&mut self`; what `&self` reaches (`fault`, `device_bytes`) only reads fields the backend never changes after creation or
// a word of page-locked memory the device writes: sharing a `&BatchDenoiser` between threads is sound.
unsafe impl Sync for BatchDenoiser {}

/// `struct nnn_batch_opts` (include/nnn_batch.h)
#[repr(C)]
#[derive(Default)]
pub struct BatchOpts {
    pub max_group_frames: c_int,
    pub reserved: [c_int; 7],
}

impl BatchDenoiser {
    /// A batch sized for calls of at most `max_group_frames` frames: a real-time host that ticks one frame per call (what
    /// `DenoiseSignal` does, src/signal.rs:102-104) passes 1 and holds 33 KB per stream instead of 360.
    pub fn sized(n_streams: usize, max_group_frames: usize, model: Option<&RnnModel>, device: i32) -> Option<BatchDenoiser> {
        let m = model.map_or(std::ptr::null(), |m| m.0 as *const RawModel);
        let n = n_streams as c_int;
        let opts = BatchOpts { max_group_frames: max_group_frames as c_int, ..Default::default() };
        let raw = unsafe { nnn_batch_create_opts(&m, &n, 1, device, &opts) };
        if raw.is_null() {
            None
        } else {
            Some(BatchDenoiser { raw, n: n_streams })
        }
    }
    pub fn device_bytes(&self) -> usize {
        unsafe { nnn_batch_device_bytes(self.raw) }
    }
    pub fn new(n_streams: usize, model: Option<&RnnModel>, device: i32) -> Option<BatchDenoiser> {
        let m = model.map_or(std::ptr::null(), |m| m.0 as *const RawModel);
        let raw = unsafe { nnn_batch_create(m, n_streams as c_int, device) };
        if raw.is_null() {
            None
        } else {
            Some(BatchDenoiser { raw, n: n_streams })
        }
    }
    /// `input`/`output`: `[n_streams][n_frames][480]`; `vad`: `[n_frames][n_streams]`.
    pub fn process(&mut self, output: &mut [f32], input: &[f32], vad: &mut [f32], n_frames: usize) {
        assert_eq!(input.len(), self.n * n_frames * DenoiseState::FRAME_SIZE);
        assert_eq!(output.len(), input.len());
        assert_eq!(vad.len(), self.n * n_frames);
        let rc = unsafe {
            nnn_batch_process_host(
                self.raw,
                input.as_ptr(),
                output.as_mut_ptr(),
                vad.as_mut_ptr(),
                n_frames as c_int,
                n_frames * DenoiseState::FRAME_SIZE,
                DenoiseState::FRAME_SIZE,
            )
        };
        assert_eq!(rc, 0, "nnnoiseless-mi355x: backend error");
    }
    /// Device-resident buffers (see include/nnn_batch.h); asynchronous.
    pub unsafe fn process_device(
        &mut self,
        d_out: *mut f32,
        d_in: *const f32,
        d_vad: *mut f32,
        n_frames: usize,
        stream_stride: usize,
        frame_stride: usize,
        hip_stream: *mut c_void,
    ) {
        let rc = nnn_batch_process_device(self.raw, d_in, d_out, d_vad, n_frames as c_int, stream_stride, frame_stride, hip_stream);
        assert_eq!(rc, 0, "nnnoiseless-mi355x: backend error");
    }
    /// The network alone (`nnn_batch_network_host`): `features` `[n_frames][n_streams][42]` (and `silence` `[n_frames][n_streams]`, 0 / 1)
    /// -> the raw gains `[n_frames][n_streams][22]` and `vad` `[n_frames][n_streams]` of every stream's resident model.  Moves the three
    /// GRU states and nothing else; any `n_frames >= 1`.
    pub fn network(&mut self, features: &[f32], silence: Option<&[i32]>, gains: &mut [f32], vad: &mut [f32], n_frames: usize) {
        assert_eq!(features.len(), self.n * n_frames * 42);
        assert_eq!(gains.len(), self.n * n_frames * 22);
        assert_eq!(vad.len(), self.n * n_frames);
        if let Some(s) = silence {
            assert_eq!(s.len(), self.n * n_frames);
        }
        let sil = silence.map_or(std::ptr::null(), |s| s.as_ptr());
        let rc = unsafe { nnn_batch_network_host(self.raw, features.as_ptr(), sil, gains.as_mut_ptr(), vad.as_mut_ptr(), n_frames as c_int) };
        assert_eq!(rc, 0, "nnnoiseless-mi355x: backend error");
    }
    /// Device-resident rows in the C call's order (see include/nnn_batch.h "Network-only calls"; `d_silence` / `d_vad` may be null);
    /// asynchronous.
    pub unsafe fn network_device(
        &mut self,
        d_features: *const f32,
        d_silence: *const i32,
        d_gains: *mut f32,
        d_vad: *mut f32,
        n_frames: usize,
        hip_stream: *mut c_void,
    ) {
        let rc = nnn_batch_network_device(self.raw, d_features, d_silence, d_gains, d_vad, n_frames as c_int, hip_stream);
        assert_eq!(rc, 0, "nnnoiseless-mi355x: backend error");
    }
    /// True once a frame hand-off inside the pitch stage has failed (sticky until `reset`): for hosts that drive
    /// `nnn_batch_process_device` on their own HIP stream and synchronise that stream themselves.
    pub fn fault(&self) -> bool {
        unsafe { nnn_batch_fault(self.raw) != 0 }
    }

    /// From the next `process` on the listed streams sit out: their state is parked, their input is not read, their rows of
    /// `output` and `vad` are left as they were, and no work is done for blocks of streams that are all held
    /// (`nnn_batch_hold_streams`).  `Err` (nothing changed) on an index out of range, a repeat or a stream already held.
    pub fn hold_streams(&mut self, streams: &[i32]) -> Result<(), ()> {
        let rc = unsafe { nnn_batch_hold_streams(self.raw, streams.as_ptr(), streams.len() as c_int) };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    /// Held streams take part again from the next `process` on, exactly as if the calls in between had not happened for them.
    pub fn resume_streams(&mut self, streams: &[i32]) -> Result<(), ()> {
        let rc = unsafe { nnn_batch_resume_streams(self.raw, streams.as_ptr(), streams.len() as c_int) };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    pub fn num_held(&self) -> usize {
        unsafe { nnn_batch_num_held(self.raw) as usize }
    }
    /// Gain floors of the listed streams (`nnn_batch_set_gain_floor`): in every `process` a non-silent frame's raw network gain becomes
    /// `max(gain, floor)` before the pitch filter and the smoothing see it.  `floors`: one value per listed stream (all its 22 bands) or
    /// 22 per stream; 0 = off; [`attenuation_limit_db`] turns "never more than 18 dB down" into a floor.  Configuration, not state:
    /// resets, imports, hold / resume leave the floors alone, `clone` copies them.  `Err` (nothing changed) on an index out of range, a
    /// repeat, a length that is neither, or a floor outside [0, 1].
    pub fn set_gain_floor(&mut self, streams: &[i32], floors: &[f32]) -> Result<(), ()> {
        let bands = if !streams.is_empty() && floors.len() == streams.len() * 22 { 22 } else { 1 };
        if floors.len() != streams.len() * bands {
            return Err(());
        }
        let rc = unsafe { nnn_batch_set_gain_floor(self.raw, streams.as_ptr(), streams.len() as c_int, floors.as_ptr(), bands as c_int) };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    /// `[streams.len() * 22]`: the listed streams' floors.
    pub fn gain_floor(&self, streams: &[i32]) -> Result<Vec<f32>, ()> {
        let mut f = vec![0f32; streams.len() * 22];
        let rc = unsafe { nnn_batch_get_gain_floor(self.raw, streams.as_ptr(), streams.len() as c_int, f.as_mut_ptr()) };
        if rc == 0 { Ok(f) } else { Err(()) }
    }
    /// Streams with any floor above 0.
    pub fn num_floored(&self) -> usize {
        unsafe { nnn_batch_num_floored(self.raw) as usize }
    }
    /// Channel link (`nnn_batch_set_channel_link`): the streams of group `s / channels` -- the channels of one stereo or four-channel
    /// group at the PCM boundary -- get one common gain per band, the largest or smallest of their network outputs, before the floor, the
    /// pitch filter and the smoothing see it; silent frames and held streams neither give nor take.  `channels` 2 or 4; 1 or
    /// `LinkMode::Off`: off.  Configuration, not state: resets, imports, hold / resume leave it alone, `clone` copies it.  `Err` (nothing
    /// changed) on other channel counts, `n_streams % channels != 0`, pending frames or a set fault.
    pub fn set_channel_link(&mut self, channels: usize, mode: LinkMode) -> Result<(), ()> {
        let rc = unsafe { nnn_batch_set_channel_link(self.raw, channels as c_int, mode as c_int) };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    /// `(channels, mode)` the next `process` runs under: `(1, LinkMode::Off)` while off.
    pub fn channel_link(&self) -> (usize, LinkMode) {
        let (mut ch, mut md): (c_int, c_int) = (1, 0);
        unsafe { nnn_batch_get_channel_link(self.raw, &mut ch, &mut md) };
        (ch as usize, match md { 1 => LinkMode::Max, 2 => LinkMode::Min, _ => LinkMode::Off })
    }
    /// `[n_streams]`: which streams are held.
    pub fn held(&self) -> Vec<bool> {
        let mut m = vec![0u8; self.n];
        let rc = unsafe { nnn_batch_held_mask(self.raw, m.as_mut_ptr(), m.len()) };
        assert_eq!(rc, 0, "nnnoiseless-mi355x: backend error");
        m.into_iter().map(|v| v != 0).collect()
    }

    pub fn reset(&mut self) {
        unsafe { nnn_batch_reset(self.raw) };
    }
}
/// `DenoiseState` is `Clone` in the reference (src/denoise.rs:36): a second batch with the same models and a device-side
/// copy of every stream's state (`nnn_batch_clone`).
impl Clone for BatchDenoiser {
    fn clone(&self) -> BatchDenoiser {
        let raw = unsafe { nnn_batch_clone(self.raw) };
        assert!(!raw.is_null(), "nnnoiseless-mi355x: clone failed");
        BatchDenoiser { raw, n: self.n }
    }
}
impl Drop for BatchDenoiser {
    fn drop(&mut self) {
        unsafe { nnn_batch_destroy(self.raw) }
    }
}

/// Streams at another sample rate in and out of a 48 kHz batch (include/nnn_rate.h): the CLI's resampler (src/nnnoiseless.rs:106-131,
/// :179-227) in front of the batch's ordinary call and the same interpolator at the inverse ratio behind it, in one asynchronous call on
/// the GPU.  The adapter carries the partial frame and both legs' histories; any chunking gives the same bits.  It borrows the batch
/// for its lifetime and drives it: reach the batch through `batch()` to reset, hold or resume streams.
pub struct RateAdapter<'b> {
    raw: *mut RawRate,
    batch: &'b mut BatchDenoiser,
}
unsafe impl<'b> Send for RateAdapter<'b> {}

impl<'b> RateAdapter<'b> {
    /// `None` where the backend refuses: a rate of 0 or 48000 (use the batch), `max_in` of 0.
    pub fn new(batch: &'b mut BatchDenoiser, source_rate: f64, max_in: usize) -> Option<RateAdapter<'b>> {
        let raw = unsafe { nnn_rate_create(batch.raw, source_rate, max_in as c_long) };
        if raw.is_null() {
            None
        } else {
            Some(RateAdapter { raw, batch })
        }
    }
    pub fn batch(&mut self) -> &mut BatchDenoiser {
        self.batch
    }
    /// Bound of the source-rate samples a call of `n_in` samples per stream can return.
    pub fn max_output(&self, n_in: usize) -> usize {
        unsafe { nnn_rate_max_output(self.raw, n_in as c_long) as usize }
    }
    /// Bound of the frames (VAD rows) such a call can complete.
    pub fn max_frames(&self, n_in: usize) -> usize {
        unsafe { nnn_rate_max_frames(self.raw, n_in as c_long) as usize }
    }
    /// 48 kHz samples of the partial frame now held.
    pub fn carried(&self) -> usize {
        unsafe { nnn_rate_carried(self.raw) as usize }
    }
    /// `input`: `[n_streams][n_in]` floats in i16 range; `output`: `[n_streams][cap_out]`, `cap_out >= max_output(n_in)`; `vad`:
    /// `[cap_frames][n_streams]`, `cap_frames >= max_frames(n_in)`.  Returns `(n_out, n_frames)`; `Err` (nothing consumed) where the
    /// backend refuses the call.
    pub fn process(&mut self, input: &[f32], n_in: usize, output: &mut [f32], vad: &mut [f32]) -> Result<(usize, usize), ()> {
        let s = self.batch.n;
        if s == 0 || input.len() != s * n_in || output.len() % s != 0 || vad.len() % s != 0 {
            return Err(());
        }
        let (mut n_out, mut n_frames): (c_long, c_int) = (0, 0);
        let rc = unsafe {
            nnn_rate_process_host(
                self.raw,
                input.as_ptr() as *const c_void,
                n_in as c_long,
                output.as_mut_ptr() as *mut c_void,
                (output.len() / s) as c_long,
                &mut n_out,
                vad.as_mut_ptr(),
                (vad.len() / s) as c_int,
                &mut n_frames,
                0,
            )
        };
        if rc == 0 { Ok((n_out as usize, n_frames as usize)) } else { Err(()) }
    }
    /// Raw device pointers, strides in elements of `format` (0 = f32 in i16 range, 1 = i16); asynchronous on `hip_stream` (null = the
    /// batch's own stream).
    ///
    /// # Safety
    /// The pointers must be device memory of the batch's device with room for the strides and capacities given.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn process_device(
        &mut self,
        d_in: *const c_void,
        n_in: usize,
        in_stride: usize,
        d_out: *mut c_void,
        cap_out: usize,
        out_stride: usize,
        d_vad: *mut c_float,
        cap_frames: usize,
        format: c_int,
        hip_stream: *mut c_void,
    ) -> Result<(usize, usize), ()> {
        let (mut n_out, mut n_frames): (c_long, c_int) = (0, 0);
        let rc = nnn_rate_process_device(
            self.raw, d_in, n_in as c_long, in_stride, d_out, cap_out as c_long, out_stride, &mut n_out, d_vad, cap_frames as c_int, &mut n_frames, format,
            hip_stream,
        );
        if rc == 0 { Ok((n_out as usize, n_frames as usize)) } else { Err(()) }
    }
    /// The adapter alone back to its fresh state.
    pub fn reset(&mut self) {
        unsafe { nnn_rate_reset(self.raw) };
    }
    /// The listed streams' histories and carried samples cleared from the next call on (beside the batch's own `reset_streams`).
    pub fn reset_streams(&mut self, streams: &[i32]) -> Result<(), ()> {
        let rc = unsafe { nnn_rate_reset_streams(self.raw, streams.as_ptr(), streams.len() as c_int) };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
}
impl<'b> Drop for RateAdapter<'b> {
    fn drop(&mut self) {
        unsafe { nnn_rate_destroy(self.raw) }
    }
}

/// Files of unequal length through one batch, slots refilled (include/nnn_pack.h): every file gets, bit for bit, what the reference CLI's
/// loop (src/nnnoiseless.rs:301-331) gives it alone -- whole frames only, the first one processed and not written -- while the batch runs
/// full.  The packer borrows the batch for its lifetime; a run leaves it with every stream it used reset and nothing held.
pub struct FilePacker<'b> {
    raw: *mut RawPack,
    batch: &'b mut BatchDenoiser,
}
unsafe impl<'b> Send for FilePacker<'b> {}

/// steps, useful, padded, held steps, launched, held frames, files placed, the largest padding of one file (include/nnn_pack.h).
pub type PackSummary = [i64; 8];

impl<'b> FilePacker<'b> {
    /// `None` where the backend refuses: `channels` that does not divide the batch's streams, `step_frames` above the batch's longest
    /// group (0 = that group), a batch with more than one model.
    pub fn new(batch: &'b mut BatchDenoiser, channels: usize, step_frames: usize) -> Option<FilePacker<'b>> {
        let raw = unsafe { nnn_pack_create(batch.raw, channels as c_int, step_frames as c_int) };
        if raw.is_null() {
            None
        } else {
            Some(FilePacker { raw, batch })
        }
    }
    pub fn batch(&mut self) -> &mut BatchDenoiser {
        self.batch
    }
    /// The plan of a run over files of `frames` WHOLE frames, in slot units: `(slot_of_file, first_step_of_file, summary)`; pure host
    /// arithmetic, the function a run itself walks.
    pub fn plan(n_slots: usize, step_frames: usize, frames: &[u64]) -> Result<(Vec<i32>, Vec<i32>, PackSummary), ()> {
        let (mut slot, mut first, mut s) = (vec![-1i32; frames.len()], vec![-1i32; frames.len()], [0i64; 8]);
        let rc = unsafe {
            nnn_pack_plan(n_slots as c_int, step_frames as c_int, frames.as_ptr(), frames.len() as c_int, slot.as_mut_ptr(), first.as_mut_ptr(), s.as_mut_ptr())
        };
        if rc == 0 { Ok((slot, first, s)) } else { Err(()) }
    }
    /// One run over host arenas of int16 samples in and out (the CLI's raw format), `vad` optional; offsets of `files` in elements.
    /// `Err` (nothing changed) where the backend refuses the run.
    pub fn run_i16(&mut self, input: &[i16], output: &mut [i16], vad: Option<&mut [f32]>, files: &[PackFile]) -> Result<PackSummary, ()> {
        let (vp, vn) = match vad {
            Some(v) => (v.as_mut_ptr(), v.len() as u64),
            None => (std::ptr::null_mut(), 0),
        };
        let rc = unsafe {
            nnn_pack_run_host(
                self.raw,
                input.as_ptr() as *const c_void,
                input.len() as u64,
                1,
                output.as_mut_ptr() as *mut c_void,
                output.len() as u64,
                1,
                vp,
                vn,
                files.as_ptr(),
                files.len() as c_int,
            )
        };
        if rc == 0 { Ok(self.last_summary()) } else { Err(()) }
    }
    /// Raw device arenas, any of the packer's formats; asynchronous on `hip_stream` (null = the batch's own stream).
    ///
    /// # Safety
    /// The pointers must be device memory of the batch's device holding the element counts given.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn run_device(
        &mut self,
        d_in: *const c_void,
        in_elems: u64,
        in_format: c_int,
        d_out: *mut c_void,
        out_elems: u64,
        out_format: c_int,
        d_vad: *mut c_float,
        vad_elems: u64,
        files: &[PackFile],
        hip_stream: *mut c_void,
    ) -> Result<PackSummary, ()> {
        let rc = nnn_pack_run_device(
            self.raw, d_in, in_elems, in_format, d_out, out_elems, out_format, d_vad, vad_elems, files.as_ptr(), files.len() as c_int, hip_stream,
        );
        if rc == 0 { Ok(self.last_summary()) } else { Err(()) }
    }
    /// The most recent run's summary, in stream units.
    pub fn last_summary(&self) -> PackSummary {
        let mut s = [0i64; 8];
        unsafe { nnn_pack_last_summary(self.raw, s.as_mut_ptr()) };
        s
    }
}
impl<'b> Drop for FilePacker<'b> {
    fn drop(&mut self) {
        unsafe { nnn_pack_destroy(self.raw) }
    }
}

/// The per-frame body of the reference's training-data generator (src/training.rs:113-160) for `n_streams` (clean, noise, mix)
/// triples (include/nnn_train.h).
pub struct TrainingFeatures {
    raw: *mut RawTrain,
    n_streams: usize,
}
unsafe impl Send for TrainingFeatures {}

/// Columns of a training row: 42 features of the mix | 22 gains | 22 noise levels | vad (src/training.rs:89).
pub const TRAIN_ROW_WIDTH: usize = 87;

impl TrainingFeatures {
    pub fn new(n_streams: usize, device: i32) -> Option<TrainingFeatures> {
        let raw = unsafe { nnn_train_create(n_streams as c_int, device as c_int) };
        if raw.is_null() {
            None
        } else {
            Some(TrainingFeatures { raw, n_streams })
        }
    }
    pub fn num_streams(&self) -> usize {
        self.n_streams
    }
    /// `signal` / `noise` / `combined`: `[n_streams][n_frames][480]`; `cutoff`, `vad`: `[n_frames][n_streams]`; `rows`: `[n_frames][n_streams][87]`.
    pub fn process(&mut self, signal: &[f32], noise: &[f32], combined: &[f32], cutoff: &[i32], vad: &[f32], rows: &mut [f32]) -> Result<(), ()> {
        let n_frames = vad.len() / self.n_streams;
        let (na, nl) = (self.n_streams * n_frames * 480, self.n_streams * n_frames);
        if signal.len() != na || noise.len() != na || combined.len() != na || cutoff.len() != nl || vad.len() != nl || rows.len() != nl * TRAIN_ROW_WIDTH {
            return Err(());
        }
        let rc = unsafe {
            nnn_train_process_host(self.raw, signal.as_ptr(), noise.as_ptr(), combined.as_ptr(), cutoff.as_ptr(), vad.as_ptr(), rows.as_mut_ptr(), n_frames as c_int)
        };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    pub fn reset(&mut self) {
        unsafe { nnn_train_reset(self.raw) };
    }
}
impl Drop for TrainingFeatures {
    fn drop(&mut self) {
        unsafe { nnn_train_destroy(self.raw) }
    }
}

/// `struct nnn_sim_params` (include/nnn_sim.h): one triple's gains, its two biquads and its band cutoff.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct SimParams {
    pub signal_gain: f32,
    pub noise_gain: f32,
    pub sig_a: [f32; 2],
    pub sig_b: [f32; 2],
    pub noise_a: [f32; 2],
    pub noise_b: [f32; 2],
    pub band_lp: i32,
}
impl Default for SimParams {
    /// `NoiseSimulator::new` (src/training.rs:300-320): gains 1, every coefficient 0, band_lp 21.
    fn default() -> SimParams {
        SimParams { signal_gain: 1.0, noise_gain: 1.0, sig_a: [0.0; 2], sig_b: [0.0; 2], noise_a: [0.0; 2], noise_b: [0.0; 2], band_lp: 21 }
    }
}

/// The generator's `NoiseSimulator` (src/training.rs:263-422) for every triple of a `TrainingFeatures`, on the device
/// (include/nnn_sim.h): two int16 arenas of clips, per-frame offsets in, training rows (or the three signals and two labels) out.
/// Offsets are `[n_frames][n_streams]` elements of the arenas.
pub struct NoiseSimulator<'t> {
    raw: *mut RawSim,
    features: &'t mut TrainingFeatures,
}
unsafe impl<'t> Send for NoiseSimulator<'t> {}

impl<'t> NoiseSimulator<'t> {
    pub fn new(features: &'t mut TrainingFeatures) -> Option<NoiseSimulator<'t>> {
        let raw = unsafe { nnn_sim_create(features.raw) };
        if raw.is_null() {
            None
        } else {
            Some(NoiseSimulator { raw, features })
        }
    }
    pub fn features(&mut self) -> &mut TrainingFeatures {
        self.features
    }
    pub fn load_signal(&mut self, pcm: &[i16]) -> Result<(), ()> {
        let rc = unsafe { nnn_sim_load(self.raw, 0, pcm.as_ptr(), pcm.len() as u64) };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    pub fn load_noise(&mut self, pcm: &[i16]) -> Result<(), ()> {
        let rc = unsafe { nnn_sim_load(self.raw, 1, pcm.as_ptr(), pcm.len() as u64) };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    /// Borrows a device buffer as arena `which` (0 signal, 1 noise).
    ///
    /// # Safety
    /// `d_pcm` must be device memory of the object's device holding `elems` int16 samples, valid until replaced or the simulator is dropped.
    pub unsafe fn adopt_device(&mut self, which: i32, d_pcm: *const i16, elems: u64) -> Result<(), ()> {
        if nnn_sim_adopt_device(self.raw, which as c_int, d_pcm, elems) == 0 { Ok(()) } else { Err(()) }
    }
    /// Parameters of the listed triples, in force from the next call's first frame; `Err` (nothing changed) for a record the backend refuses.
    pub fn set_params(&mut self, streams: &[i32], recs: &[SimParams]) -> Result<(), ()> {
        if streams.len() != recs.len() {
            return Err(());
        }
        let rc = unsafe { nnn_sim_set_params(self.raw, streams.as_ptr(), streams.len() as c_int, recs.as_ptr()) };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    pub fn params(&mut self, streams: &[i32]) -> Result<Vec<SimParams>, ()> {
        let mut recs = vec![SimParams::default(); streams.len()];
        let rc = unsafe { nnn_sim_get_params(self.raw, streams.as_ptr(), streams.len() as c_int, recs.as_mut_ptr()) };
        if rc == 0 { Ok(recs) } else { Err(()) }
    }
    /// Rows `[n_frames][n_streams][87]` for the named frames; an offset that leaves its arena refuses the call.
    pub fn process(&mut self, sig_off: &[u64], noise_off: &[u64], rows: &mut [f32]) -> Result<(), ()> {
        let s = self.features.n_streams;
        if sig_off.len() != noise_off.len() || sig_off.len() % s != 0 || rows.len() != sig_off.len() * TRAIN_ROW_WIDTH {
            return Err(());
        }
        let rc = unsafe { nnn_sim_process_host(self.raw, sig_off.as_ptr(), noise_off.as_ptr(), rows.as_mut_ptr(), (sig_off.len() / s) as c_int) };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    /// The three signals `[n_streams][n_frames][480]` and the two labels `[n_frames][n_streams]` without the rows.
    #[allow(clippy::too_many_arguments)]
    pub fn signals(&mut self, sig_off: &[u64], noise_off: &[u64], signal: &mut [f32], noise: &mut [f32], combined: &mut [f32], cutoff: &mut [i32], vad: &mut [f32]) -> Result<(), ()> {
        let (s, nl) = (self.features.n_streams, sig_off.len());
        if noise_off.len() != nl || nl % s != 0 || signal.len() != nl * 480 || noise.len() != nl * 480 || combined.len() != nl * 480 || cutoff.len() != nl || vad.len() != nl {
            return Err(());
        }
        let rc = unsafe {
            nnn_sim_signals_host(self.raw, sig_off.as_ptr(), noise_off.as_ptr(), signal.as_mut_ptr(), noise.as_mut_ptr(), combined.as_mut_ptr(), cutoff.as_mut_ptr(), vad.as_mut_ptr(), (nl / s) as c_int)
        };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    /// Raw device pointers; asynchronous on `hip_stream` (null = the training object's own stream).
    ///
    /// # Safety
    /// The pointers must be device memory of the object's device: `n_frames x n_streams` offsets each, `n_frames x n_streams x 87` floats.
    pub unsafe fn process_device(&mut self, d_sig_off: *const u64, d_noise_off: *const u64, d_rows: *mut c_float, n_frames: usize, hip_stream: *mut c_void) -> Result<(), ()> {
        if nnn_sim_process_device(self.raw, d_sig_off, d_noise_off, d_rows, n_frames as c_int, hip_stream) == 0 { Ok(()) } else { Err(()) }
    }
    /// Filter memories and VAD counters to zero; parameters and arenas stay.  Pair with `TrainingFeatures::reset`.
    pub fn reset(&mut self) {
        unsafe { nnn_sim_reset(self.raw) };
    }
    /// A device call met a frame outside its arena (it read as zeros).
    pub fn fault(&mut self) -> bool {
        unsafe { nnn_sim_fault(self.raw) > 0 }
    }
}
impl<'t> Drop for NoiseSimulator<'t> {
    fn drop(&mut self) {
        unsafe { nnn_sim_destroy(self.raw) }
    }
}

/// `struct nnn_fit_settings` (include/nnn_fit.h): Adam as Keras runs it, the L2 factor of the GRU matrices and the clip.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct FitSettings {
    pub lr: c_float,
    pub beta1: c_float,
    pub beta2: c_float,
    pub epsilon: c_float,
    pub reg: c_float,
    pub clip: c_float,
}

/// `{total, 10 mean(w Lg), 0.5 mean(w Lv), reg term, mean(w msse)}` of the last loss or grad call.
pub type FitLosses = [f32; 5];

/// The reference's `train/rnn_train.py` and `dump_rnn.py` on the device (include/nnn_fit.h): forward pass, loss, back-propagation
/// through time and Adam for the 3-GRU network.  Rows are dense `[window][n_seq][87]`, weights `[window][n_seq]`.
pub struct Trainer {
    raw: *mut RawFit,
}
unsafe impl Send for Trainer {}

impl Trainer {
    pub const PARAMS: usize = 87503;
    pub const RNN_BYTES: usize = 87521;
    /// `template`: a `.rnn` file (its activations, its weights / 256 as the start) or `None` for the reference's training set-up
    /// with zero parameters, to be overwritten by `set_params`.
    pub fn new(template: Option<&[u8]>, max_seq: usize, max_window: usize, device: i32) -> Option<Trainer> {
        let (p, n) = template.map_or((std::ptr::null(), 0), |t| (t.as_ptr(), t.len()));
        let raw = unsafe { nnn_fit_create(p, n, max_seq as c_int, max_window as c_int, device as c_int) };
        if raw.is_null() {
            None
        } else {
            Some(Trainer { raw })
        }
    }
    /// Selector 0: parameters, 1: gradient, 2 and 3: Adam's moments.
    pub fn get(&mut self, which: i32) -> Result<Vec<f32>, ()> {
        let mut v = vec![0.0f32; Self::PARAMS];
        if unsafe { nnn_fit_get(self.raw, which as c_int, v.as_mut_ptr()) } == 0 { Ok(v) } else { Err(()) }
    }
    pub fn set(&mut self, which: i32, values: &[f32]) -> Result<(), ()> {
        assert_eq!(values.len(), Self::PARAMS);
        if unsafe { nnn_fit_set(self.raw, which as c_int, values.as_ptr()) } == 0 { Ok(()) } else { Err(()) }
    }
    pub fn params(&mut self) -> Result<Vec<f32>, ()> {
        self.get(0)
    }
    pub fn set_params(&mut self, values: &[f32]) -> Result<(), ()> {
        self.set(0, values)
    }
    pub fn step_count(&mut self) -> i64 {
        let mut n = 0i64;
        unsafe { nnn_fit_get_step(self.raw, &mut n) };
        n
    }
    pub fn set_step_count(&mut self, n: i64) -> Result<(), ()> {
        if unsafe { nnn_fit_set_step(self.raw, n) } == 0 { Ok(()) } else { Err(()) }
    }
    pub fn settings(&mut self) -> FitSettings {
        let mut s = FitSettings { lr: 0.0, beta1: 0.0, beta2: 0.0, epsilon: 0.0, reg: 0.0, clip: 0.0 };
        unsafe { nnn_fit_get_settings(self.raw, &mut s) };
        s
    }
    pub fn set_settings(&mut self, s: &FitSettings) -> Result<(), ()> {
        if unsafe { nnn_fit_set_settings(self.raw, s) } == 0 { Ok(()) } else { Err(()) }
    }
    /// The `.rnn` file of the current parameters (`clamp(rint(256 x), -128, 127)` behind the template's headers).
    pub fn export_rnn(&mut self) -> Result<Vec<u8>, ()> {
        let mut out = vec![0u8; Self::RNN_BYTES];
        if unsafe { nnn_fit_export_rnn(self.raw, out.as_mut_ptr(), out.len()) } == 0 { Ok(out) } else { Err(()) }
    }
    pub fn forward(&mut self, rows: &[f32], n_seq: usize, window: usize, gains: &mut [f32], vad: &mut [f32]) -> Result<(), ()> {
        assert!(rows.len() == n_seq * window * 87 && gains.len() == n_seq * window * 22 && vad.len() == n_seq * window);
        let rc = unsafe { nnn_fit_forward_host(self.raw, rows.as_ptr(), n_seq as c_int, window as c_int, gains.as_mut_ptr(), vad.as_mut_ptr()) };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    pub fn loss(&mut self, rows: &[f32], w: Option<&[f32]>, n_seq: usize, window: usize) -> Result<FitLosses, ()> {
        assert!(rows.len() == n_seq * window * 87 && w.map_or(true, |w| w.len() == n_seq * window));
        let rc = unsafe { nnn_fit_loss_host(self.raw, rows.as_ptr(), w.map_or(std::ptr::null(), |w| w.as_ptr()), n_seq as c_int, window as c_int) };
        if rc == 0 { self.losses() } else { Err(()) }
    }
    /// Forward pass, loss terms and the gradient into the object.
    pub fn grad(&mut self, rows: &[f32], w: Option<&[f32]>, n_seq: usize, window: usize) -> Result<FitLosses, ()> {
        assert!(rows.len() == n_seq * window * 87 && w.map_or(true, |w| w.len() == n_seq * window));
        let rc = unsafe { nnn_fit_grad_host(self.raw, rows.as_ptr(), w.map_or(std::ptr::null(), |w| w.as_ptr()), n_seq as c_int, window as c_int) };
        if rc == 0 { self.losses() } else { Err(()) }
    }
    /// One Adam step from the held gradient, then the clip.
    pub fn step(&mut self) -> Result<(), ()> {
        if unsafe { nnn_fit_step(self.raw, std::ptr::null_mut()) } == 0 { Ok(()) } else { Err(()) }
    }
    pub fn losses(&mut self) -> Result<FitLosses, ()> {
        let mut v = [0.0f32; 5];
        if unsafe { nnn_fit_losses(self.raw, v.as_mut_ptr()) } == 0 { Ok(v) } else { Err(()) }
    }
}
impl Drop for Trainer {
    fn drop(&mut self) {
        unsafe { nnn_fit_destroy(self.raw) }
    }
}

/// Per-stream sums between a reference and a test signal, carried across calls on the device (include/nnn_score.h): per stream
/// `[A, B, C, E] = [sum r^2, sum y^2, sum r y, sum (r - y)^2]` in f64 in one fixed order, the reference delayed by the stream's delay.
/// Host buffers are dense `[n_streams][n_frames][480]`, the mask `[n_frames][n_streams]`, frame sums `[n_frames][n_streams][4]`.
pub struct Scorer {
    raw: *mut RawScore,
    n_streams: usize,
}
unsafe impl Send for Scorer {}

impl Scorer {
    pub const MAX_DELAY: usize = 960;
    pub fn new(n_streams: usize, max_delay: usize, device: i32) -> Option<Scorer> {
        let raw = unsafe { nnn_score_create(n_streams as c_int, max_delay as c_int, device as c_int) };
        if raw.is_null() {
            None
        } else {
            Some(Scorer { raw, n_streams })
        }
    }
    pub fn num_streams(&self) -> usize {
        self.n_streams
    }
    /// Delays of the listed streams (`None`: one per stream); also zeroes their history, totals and count.
    pub fn set_delay(&mut self, idx: Option<&[i32]>, delays: &[i32]) -> Result<(), ()> {
        assert_eq!(delays.len(), idx.map_or(self.n_streams, |i| i.len()));
        let rc = unsafe { nnn_score_set_delay(self.raw, idx.map_or(std::ptr::null(), |i| i.as_ptr()), delays.len() as c_int, delays.as_ptr()) };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    pub fn delay(&mut self) -> Vec<i32> {
        let mut d = vec![0i32; self.n_streams];
        unsafe { nnn_score_get_delay(self.raw, std::ptr::null(), self.n_streams as c_int, d.as_mut_ptr()) };
        d
    }
    /// History, totals and count of the listed streams (`None`: all) to zero; the delays stay.
    pub fn reset(&mut self, idx: Option<&[i32]>) -> Result<(), ()> {
        let rc = unsafe { nnn_score_reset(self.raw, idx.map_or(std::ptr::null(), |i| i.as_ptr()), idx.map_or(0, |i| i.len()) as c_int) };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    pub fn accumulate(&mut self, reference: &[f32], test: &[f32], n_frames: usize, valid: Option<&[u8]>, frame_sums: Option<&mut [f64]>) -> Result<(), ()> {
        let rows = self.n_streams * n_frames;
        assert!(reference.len() == rows * 480 && test.len() == rows * 480 && valid.map_or(true, |v| v.len() == rows));
        assert!(frame_sums.as_ref().map_or(true, |f| f.len() == rows * 4));
        let rc = unsafe {
            nnn_score_accumulate_host(
                self.raw,
                reference.as_ptr(),
                test.as_ptr(),
                valid.map_or(std::ptr::null(), |v| v.as_ptr()),
                frame_sums.map_or(std::ptr::null_mut(), |f| f.as_mut_ptr()),
                n_frames as c_int,
            )
        };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    /// Raw device pointers, asynchronous on `hip_stream` (null: the scorer's own stream); strides in floats.
    ///
    /// # Safety
    /// The pointers must be device memory of the sizes include/nnn_score.h states, valid until the call has run.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn accumulate_device(
        &mut self,
        d_ref: *const f32,
        d_test: *const f32,
        d_valid: *const u8,
        d_frame_sums: *mut f64,
        n_frames: usize,
        stream_stride: usize,
        frame_stride: usize,
        hip_stream: *mut c_void,
    ) -> Result<(), ()> {
        let rc = nnn_score_accumulate_device(self.raw, d_ref, d_test, d_valid, d_frame_sums, n_frames as c_int, stream_stride, frame_stride, hip_stream);
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    /// `([n_streams][4] sums, [n_streams] frames counted)`; waits for the calls made so far.
    pub fn totals(&mut self) -> Result<(Vec<[f64; 4]>, Vec<u64>), ()> {
        let mut t = vec![[0.0f64; 4]; self.n_streams];
        let mut c = vec![0u64; self.n_streams];
        if unsafe { nnn_score_totals(self.raw, t.as_mut_ptr() as *mut f64, c.as_mut_ptr()) } == 0 { Ok((t, c)) } else { Err(()) }
    }
    /// # Safety
    /// Device memory for `[n_streams][4]` doubles and `[n_streams]` counts (either may be null).
    pub unsafe fn totals_device(&mut self, d_out: *mut f64, d_counts: *mut u64, hip_stream: *mut c_void) -> Result<(), ()> {
        if nnn_score_totals_device(self.raw, d_out, d_counts, hip_stream) == 0 { Ok(()) } else { Err(()) }
    }
    /// `10 log10(A / E)`; inf or nan for zero denominators, as IEEE division and the logarithm give.
    pub fn snr_db(a: f64, e: f64) -> f64 {
        10.0 * (a / e).log10()
    }
    /// `10 log10(C^2 / (A B - C^2))`.
    pub fn si_sdr_db(a: f64, b: f64, c: f64) -> f64 {
        10.0 * (c * c / (a * b - c * c)).log10()
    }
}
impl Drop for Scorer {
    fn drop(&mut self) {
        unsafe { nnn_score_destroy(self.raw) }
    }
}

/// The VAD gate behind the denoiser (include/nnn_gate.h): per stream a threshold on the speech probability, a grace period, a look-back
/// that delays the audio a few frames so the onset is not cut, and a gain for the closed gate (0 = mute).  Host buffers are dense
/// `[n_streams][n_frames][480]`, VAD and open flags `[n_frames][n_streams]`, the live mask `[n_streams]`.
pub struct VadGate {
    raw: *mut RawGate,
    n_streams: usize,
}
unsafe impl Send for VadGate {}

impl VadGate {
    pub const MAX_LOOKBACK: usize = 8;
    pub const MAX_GRACE: usize = 6000;
    pub fn new(n_streams: usize, max_lookback: usize, device: i32) -> Option<VadGate> {
        let raw = unsafe { nnn_gate_create(n_streams as c_int, max_lookback as c_int, device as c_int) };
        if raw.is_null() {
            None
        } else {
            Some(VadGate { raw, n_streams })
        }
    }
    pub fn num_streams(&self) -> usize {
        self.n_streams
    }
    /// Bytes of one exported record.
    pub fn state_bytes(&self) -> usize {
        unsafe { nnn_gate_state_bytes(self.raw) }
    }
    /// Parameters of the listed streams (`None`: one per stream); also resets those streams.
    pub fn set_params(&mut self, idx: Option<&[i32]>, params: &[GateParams]) -> Result<(), ()> {
        assert_eq!(params.len(), idx.map_or(self.n_streams, |i| i.len()));
        let rc = unsafe { nnn_gate_set_params(self.raw, idx.map_or(std::ptr::null(), |i| i.as_ptr()), params.len() as c_int, params.as_ptr()) };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    pub fn params(&mut self) -> Vec<GateParams> {
        let mut p = vec![GateParams::default(); self.n_streams];
        unsafe { nnn_gate_get_params(self.raw, std::ptr::null(), self.n_streams as c_int, p.as_mut_ptr()) };
        p
    }
    /// The listed streams (`None`: all) back to "never voiced, closed, no history"; the parameters stay.
    pub fn reset(&mut self, idx: Option<&[i32]>) -> Result<(), ()> {
        let rc = unsafe { nnn_gate_reset(self.raw, idx.map_or(std::ptr::null(), |i| i.as_ptr()), idx.map_or(0, |i| i.len()) as c_int) };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    /// In place on host memory; what a stream marked 0 in `live` owns is left as it was.
    pub fn apply(&mut self, audio: &mut [f32], vad: &[f32], n_frames: usize, live: Option<&[u8]>, open: Option<&mut [u8]>) -> Result<(), ()> {
        let rows = self.n_streams * n_frames;
        assert!(audio.len() == rows * 480 && vad.len() == rows && live.map_or(true, |l| l.len() == self.n_streams));
        assert!(open.as_ref().map_or(true, |o| o.len() == rows));
        let rc = unsafe {
            nnn_gate_apply_host(
                self.raw,
                audio.as_ptr(),
                audio.as_mut_ptr(),
                vad.as_ptr(),
                live.map_or(std::ptr::null(), |l| l.as_ptr()),
                open.map_or(std::ptr::null_mut(), |o| o.as_mut_ptr()),
                n_frames as c_int,
            )
        };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    /// Raw device pointers, asynchronous on `hip_stream` (null: the gate's own stream); strides in floats; `d_out == d_in` is in place.
    ///
    /// # Safety
    /// The pointers must be device memory of the sizes include/nnn_gate.h states, valid until the call has run.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn apply_device(
        &mut self,
        d_in: *const f32,
        d_out: *mut f32,
        d_vad: *const f32,
        d_live: *const u8,
        d_open: *mut u8,
        n_frames: usize,
        stream_stride: usize,
        frame_stride: usize,
        hip_stream: *mut c_void,
    ) -> Result<(), ()> {
        let rc = nnn_gate_apply_device(self.raw, d_in, d_out, d_vad, d_live, d_open, n_frames as c_int, stream_stride, frame_stride, hip_stream);
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    /// The packed boundary of `BatchDenoiser::process_pcm_device`.
    ///
    /// # Safety
    /// As `apply_device`, in elements of the layout's format.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn apply_pcm_device(
        &mut self,
        d_in: *const c_void,
        d_out: *mut c_void,
        d_vad: *const f32,
        d_live: *const u8,
        d_open: *mut u8,
        n_frames: usize,
        layout: &PcmLayout,
        hip_stream: *mut c_void,
    ) -> Result<(), ()> {
        let rc = nnn_gate_apply_pcm_device(self.raw, d_in, d_out, d_vad, d_live, d_open, n_frames as c_int, layout, hip_stream);
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    /// Records of `state_bytes()` bytes each: a stream moved to another gate continues bit for bit.
    pub fn export_streams(&mut self, idx: &[i32]) -> Result<Vec<u8>, ()> {
        let mut rec = vec![0u8; idx.len() * self.state_bytes()];
        let rc = unsafe { nnn_gate_export_streams(self.raw, idx.as_ptr(), idx.len() as c_int, rec.as_mut_ptr() as *mut c_void, rec.len()) };
        if rc == 0 { Ok(rec) } else { Err(()) }
    }
    pub fn import_streams(&mut self, idx: &[i32], records: &[u8]) -> Result<(), ()> {
        let rc = unsafe { nnn_gate_import_streams(self.raw, idx.as_ptr(), idx.len() as c_int, records.as_ptr() as *const c_void, records.len()) };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
}
impl Drop for VadGate {
    fn drop(&mut self) {
        unsafe { nnn_gate_destroy(self.raw) }
    }
}

/// The conference mixer behind the gate (include/nnn_mix.h): per stream a room and a gain; every live member of a room receives the sum
/// of the room's other talkers (mix-minus).  Host buffers are dense `[n_streams][n_frames][480]`, talk flags (the gate's open flags) and
/// heard counts `[n_frames][n_streams]`, the live mask `[n_streams]`.
pub struct Mixer {
    raw: *mut RawMix,
    n_streams: usize,
}
unsafe impl Send for Mixer {}

impl Mixer {
    pub const MAX_GAIN: f32 = 16.0;
    pub fn new(n_streams: usize, device: i32) -> Option<Mixer> {
        let raw = unsafe { nnn_mix_create(n_streams as c_int, device as c_int) };
        if raw.is_null() {
            None
        } else {
            Some(Mixer { raw, n_streams })
        }
    }
    pub fn num_streams(&self) -> usize {
        self.n_streams
    }
    /// Rooms of the listed streams (`None`: one per stream), -1 = alone; in force from the next call.  Leaves the ramp state alone: mute a
    /// stream before moving it.
    pub fn set_rooms(&mut self, idx: Option<&[i32]>, room: &[i32]) -> Result<(), ()> {
        assert_eq!(room.len(), idx.map_or(self.n_streams, |i| i.len()));
        let rc = unsafe { nnn_mix_set_rooms(self.raw, idx.map_or(std::ptr::null(), |i| i.as_ptr()), room.len() as c_int, room.as_ptr()) };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    /// Gains of the listed streams in `[0, MAX_GAIN]`; a change reaches the audio through a one-frame ramp.
    pub fn set_gains(&mut self, idx: Option<&[i32]>, gain: &[f32]) -> Result<(), ()> {
        assert_eq!(gain.len(), idx.map_or(self.n_streams, |i| i.len()));
        let rc = unsafe { nnn_mix_set_gains(self.raw, idx.map_or(std::ptr::null(), |i| i.as_ptr()), gain.len() as c_int, gain.as_ptr()) };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    pub fn rooms(&mut self) -> Vec<i32> {
        let mut r = vec![0i32; self.n_streams];
        unsafe { nnn_mix_get_rooms(self.raw, std::ptr::null(), self.n_streams as c_int, r.as_mut_ptr()) };
        r
    }
    pub fn gains(&mut self) -> Vec<f32> {
        let mut g = vec![0f32; self.n_streams];
        unsafe { nnn_mix_get_gains(self.raw, std::ptr::null(), self.n_streams as c_int, g.as_mut_ptr()) };
        g
    }
    /// The listed streams (`None`: all) back to "silent so far"; rooms and gains stay.
    pub fn reset(&mut self, idx: Option<&[i32]>) -> Result<(), ()> {
        let rc = unsafe { nnn_mix_reset(self.raw, idx.map_or(std::ptr::null(), |i| i.as_ptr()), idx.map_or(0, |i| i.len()) as c_int) };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    /// Host memory, never in place; what a stream marked 0 in `live` owns in `out` and `heard` is left as it was.
    pub fn apply(&mut self, input: &[f32], out: &mut [f32], n_frames: usize, talk: Option<&[u8]>, live: Option<&[u8]>, heard: Option<&mut [i32]>) -> Result<(), ()> {
        let rows = self.n_streams * n_frames;
        assert!(input.len() == rows * 480 && out.len() == rows * 480 && talk.map_or(true, |t| t.len() == rows));
        assert!(live.map_or(true, |l| l.len() == self.n_streams) && heard.as_ref().map_or(true, |h| h.len() == rows));
        let rc = unsafe {
            nnn_mix_apply_host(
                self.raw,
                input.as_ptr(),
                out.as_mut_ptr(),
                talk.map_or(std::ptr::null(), |t| t.as_ptr()),
                live.map_or(std::ptr::null(), |l| l.as_ptr()),
                heard.map_or(std::ptr::null_mut(), |h| h.as_mut_ptr()),
                n_frames as c_int,
            )
        };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    /// Raw device pointers, asynchronous on `hip_stream` (null: the mixer's own stream); strides in floats, a pair per side.
    ///
    /// # Safety
    /// The pointers must be device memory of the sizes include/nnn_mix.h states, valid until the call has run; `d_out` must not overlap `d_in`.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn apply_device(
        &mut self,
        d_in: *const f32,
        d_out: *mut f32,
        d_talk: *const u8,
        d_live: *const u8,
        d_heard: *mut i32,
        n_frames: usize,
        in_strides: (usize, usize),
        out_strides: (usize, usize),
        hip_stream: *mut c_void,
    ) -> Result<(), ()> {
        let rc = nnn_mix_apply_device(self.raw, d_in, d_out, d_talk, d_live, d_heard, n_frames as c_int, in_strides.0, in_strides.1, out_strides.0, out_strides.1, hip_stream);
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    /// The packed boundary of `BatchDenoiser::process_pcm_device`, a layout (and format) per side.
    ///
    /// # Safety
    /// As `apply_device`, in elements of each layout's format.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn apply_pcm_device(
        &mut self,
        d_in: *const c_void,
        d_out: *mut c_void,
        d_talk: *const u8,
        d_live: *const u8,
        d_heard: *mut i32,
        n_frames: usize,
        in_layout: &PcmLayout,
        out_layout: &PcmLayout,
        hip_stream: *mut c_void,
    ) -> Result<(), ()> {
        let rc = nnn_mix_apply_pcm_device(self.raw, d_in, d_out, d_talk, d_live, d_heard, n_frames as c_int, in_layout, out_layout, hip_stream);
        if rc == 0 { Ok(()) } else { Err(()) }
    }
}
impl Drop for Mixer {
    fn drop(&mut self) {
        unsafe { nnn_mix_destroy(self.raw) }
    }
}

/// The talker picker between the gate and the mixer (include/nnn_pick.h): per stream a room and a pin, per object `k`, `decay` and
/// `stick`; of every room's open gates the `k` loudest talk, and an incumbent keeps its place until a challenger is `stick` times louder.
/// Host audio is dense `[n_streams][n_frames][480]`; open flags (the gate's), talk flags (what `Mixer::apply` takes), dominant indices and
/// levels are `[n_frames][n_streams]`, the live mask `[n_streams]`.
pub struct Picker {
    raw: *mut RawPick,
    n_streams: usize,
}
unsafe impl Send for Picker {}

impl Picker {
    pub const MAX_K: i32 = 8;
    pub const MAX_STICK: f32 = 16.0;
    pub fn new(n_streams: usize, device: i32) -> Option<Picker> {
        let raw = unsafe { nnn_pick_create(n_streams as c_int, device as c_int) };
        if raw.is_null() {
            None
        } else {
            Some(Picker { raw, n_streams })
        }
    }
    pub fn num_streams(&self) -> usize {
        self.n_streams
    }
    /// Rooms of the listed streams (`None`: one per stream), -1 = alone: the mixer's labels; in force from the next call.
    pub fn set_rooms(&mut self, idx: Option<&[i32]>, room: &[i32]) -> Result<(), ()> {
        assert_eq!(room.len(), idx.map_or(self.n_streams, |i| i.len()));
        let rc = unsafe { nnn_pick_set_rooms(self.raw, idx.map_or(std::ptr::null(), |i| i.as_ptr()), room.len() as c_int, room.as_ptr()) };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    /// Pins of the listed streams, each 0 or 1: a pinned stream with an open gate ranks ahead of every unpinned one.
    pub fn set_pinned(&mut self, idx: Option<&[i32]>, pinned: &[u8]) -> Result<(), ()> {
        assert_eq!(pinned.len(), idx.map_or(self.n_streams, |i| i.len()));
        let rc = unsafe { nnn_pick_set_pinned(self.raw, idx.map_or(std::ptr::null(), |i| i.as_ptr()), pinned.len() as c_int, pinned.as_ptr()) };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    /// `k` in `1 ..= MAX_K`, `decay` in `[0, 1]`, `stick` in `[1, MAX_STICK]`.
    pub fn set_policy(&mut self, k: i32, decay: f32, stick: f32) -> Result<(), ()> {
        let rc = unsafe { nnn_pick_set_policy(self.raw, k as c_int, decay, stick) };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    pub fn rooms(&mut self) -> Vec<i32> {
        let mut r = vec![0i32; self.n_streams];
        unsafe { nnn_pick_get_rooms(self.raw, std::ptr::null(), self.n_streams as c_int, r.as_mut_ptr()) };
        r
    }
    pub fn pinned(&mut self) -> Vec<u8> {
        let mut p = vec![0u8; self.n_streams];
        unsafe { nnn_pick_get_pinned(self.raw, std::ptr::null(), self.n_streams as c_int, p.as_mut_ptr()) };
        p
    }
    pub fn policy(&mut self) -> (i32, f32, f32) {
        let (mut k, mut decay, mut stick) = (0 as c_int, 0f32, 0f32);
        unsafe { nnn_pick_get_policy(self.raw, &mut k, &mut decay, &mut stick) };
        (k as i32, decay, stick)
    }
    /// The listed streams (`None`: all) back to "silent and not selected so far"; rooms, pins and policy stay.
    pub fn reset(&mut self, idx: Option<&[i32]>) -> Result<(), ()> {
        let rc = unsafe { nnn_pick_reset(self.raw, idx.map_or(std::ptr::null(), |i| i.as_ptr()), idx.map_or(0, |i| i.len()) as c_int) };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    /// Host memory; what a stream marked 0 in `live` owns in `talk`, `dominant` and `level` is left as it was.
    #[allow(clippy::too_many_arguments)]
    pub fn select(&mut self, input: &[f32], talk: &mut [u8], n_frames: usize, open: Option<&[u8]>, live: Option<&[u8]>, dominant: Option<&mut [i32]>, level: Option<&mut [f64]>) -> Result<(), ()> {
        let rows = self.n_streams * n_frames;
        assert!(input.len() == rows * 480 && talk.len() == rows && open.map_or(true, |o| o.len() == rows));
        assert!(live.map_or(true, |l| l.len() == self.n_streams) && dominant.as_ref().map_or(true, |d| d.len() == rows) && level.as_ref().map_or(true, |l| l.len() == rows));
        let rc = unsafe {
            nnn_pick_select_host(
                self.raw,
                input.as_ptr(),
                open.map_or(std::ptr::null(), |o| o.as_ptr()),
                live.map_or(std::ptr::null(), |l| l.as_ptr()),
                talk.as_mut_ptr(),
                dominant.map_or(std::ptr::null_mut(), |d| d.as_mut_ptr()),
                level.map_or(std::ptr::null_mut(), |l| l.as_mut_ptr()),
                n_frames as c_int,
            )
        };
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    /// Raw device pointers, asynchronous on `hip_stream` (null: the picker's own stream); strides in floats; `d_talk` may be `d_open` itself.
    ///
    /// # Safety
    /// The pointers must be device memory of the sizes include/nnn_pick.h states, valid until the call has run.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn select_device(
        &mut self,
        d_in: *const f32,
        d_open: *const u8,
        d_live: *const u8,
        d_talk: *mut u8,
        d_dominant: *mut i32,
        d_level: *mut f64,
        n_frames: usize,
        strides: (usize, usize),
        hip_stream: *mut c_void,
    ) -> Result<(), ()> {
        let rc = nnn_pick_select_device(self.raw, d_in, d_open, d_live, d_talk, d_dominant, d_level, n_frames as c_int, strides.0, strides.1, hip_stream);
        if rc == 0 { Ok(()) } else { Err(()) }
    }
    /// The packed boundary of `BatchDenoiser::process_pcm_device`.
    ///
    /// # Safety
    /// As `select_device`, in elements of the layout's format.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn select_pcm_device(
        &mut self,
        d_in: *const c_void,
        d_open: *const u8,
        d_live: *const u8,
        d_talk: *mut u8,
        d_dominant: *mut i32,
        d_level: *mut f64,
        n_frames: usize,
        layout: &PcmLayout,
        hip_stream: *mut c_void,
    ) -> Result<(), ()> {
        let rc = nnn_pick_select_pcm_device(self.raw, d_in, d_open, d_live, d_talk, d_dominant, d_level, n_frames as c_int, layout, hip_stream);
        if rc == 0 { Ok(()) } else { Err(()) }
    }
}
impl Drop for Picker {
    fn drop(&mut self) {
        unsafe { nnn_pick_destroy(self.raw) }
    }
}

/// Same surface as `nnnoiseless::DenoiseState<'model>` (src/denoise.rs:36-116), lifetime and `Clone` included: host code that names
/// `DenoiseState<'static>` or borrows a model for `'model` compiles unchanged.  The backend copies the model to the device when the
/// state is made, so the borrow is only a marker (`PhantomData`): it keeps the reference's rule that a borrowed model outlives the
/// states made from it, without holding a pointer to it.
#[derive(Clone)]
pub struct DenoiseState<'model> {
    batch: BatchDenoiser,
    _model: std::marker::PhantomData<&'model RnnModel>,
}

impl DenoiseState<'static> {
    /// A `DenoiseState` processes this many samples at a time.
    pub const FRAME_SIZE: usize = 480;

    /// `DenoiseState::new()` (src/denoise.rs:53-55): the built-in model.
    pub fn new() -> Box<DenoiseState<'static>> {
        Box::new(DenoiseState { batch: BatchDenoiser::sized(1, 1, None, 0).expect("no MI355X backend"), _model: std::marker::PhantomData })
    }
    /// `DenoiseState::from_model(model)` (src/denoise.rs:61-63): the state owns the model (here: its device copy; the host copy is dropped).
    pub fn from_model(model: RnnModel) -> Box<DenoiseState<'static>> {
        Box::new(DenoiseState { batch: BatchDenoiser::sized(1, 1, Some(&model), 0).expect("no MI355X backend"), _model: std::marker::PhantomData })
    }
}

impl<'model> DenoiseState<'model> {
    /// `DenoiseState::with_model(&model)` (src/denoise.rs:72-74): the same model shared between states.
    pub fn with_model(model: &'model RnnModel) -> Box<DenoiseState<'model>> {
        Box::new(DenoiseState { batch: BatchDenoiser::sized(1, 1, Some(model), 0).expect("no MI355X backend"), _model: std::marker::PhantomData })
    }
    /// src/denoise.rs:95-116: 480 samples in the range of an i16 in, 480 out, returns the voice-activity probability.
    pub fn process_frame(&mut self, output: &mut [f32], input: &[f32]) -> f32 {
        assert!(input.len() == DenoiseState::FRAME_SIZE); // src/features.rs:98
        let mut vad = [0.0f32];
        self.batch.process(&mut output[..DenoiseState::FRAME_SIZE], input, &mut vad, 1);
        vad[0]
    }
}

/// `nnnoiseless::DenoiseSignal` (src/signal.rs:29-138) over one batch: the per-channel loop of `refill_out_bufs`
/// (src/signal.rs:102-104) is one call on a batch of `CHANNELS` streams.  Needs the `dasp` feature, like the reference's.
#[cfg(feature = "dasp")]
pub mod signal {
    use super::{BatchDenoiser, DenoiseState, RnnModel};
    use dasp::frame::Frame;
    use dasp::sample::Sample;
    use dasp::signal::Signal;

    const FRAME_SIZE: usize = 480;

    #[derive(Clone)]
    pub struct DenoiseSignal<'model, S: Signal> {
        input: S,
        states: BatchDenoiser,               // CHANNELS streams in lock-step
        in_bufs: Vec<f32>,                   // [channel][480]
        out_bufs: Vec<f32>,
        vad: Vec<f32>,
        out_idx: usize,
        _model: std::marker::PhantomData<&'model RnnModel>,
    }

    impl<'model, S: Signal> DenoiseSignal<'model, S> {
        fn make(input: S, model: Option<&RnnModel>) -> Self {
            let ch = S::Frame::CHANNELS;
            DenoiseSignal {
                input,
                states: BatchDenoiser::sized(ch, 1, model, 0).expect("no MI355X backend"),
                in_bufs: vec![0.0; ch * FRAME_SIZE],
                out_bufs: vec![0.0; ch * FRAME_SIZE],
                vad: vec![0.0; ch],
                out_idx: 0,
                _model: std::marker::PhantomData,
            }
            .discard_first_frame()
        }
        /// src/signal.rs:39-48
        pub fn new(input: S) -> DenoiseSignal<'static, S> {
            DenoiseSignal::<'static, S>::make(input, None)
        }
        /// src/signal.rs:55-64
        pub fn with_model(input: S, model: &'model RnnModel) -> DenoiseSignal<'model, S> {
            Self::make(input, Some(model))
        }
        /// src/signal.rs:72-81
        pub fn from_model(input: S, model: RnnModel) -> DenoiseSignal<'static, S> {
            DenoiseSignal::<'static, S>::make(input, Some(&model))
        }
        fn discard_first_frame(mut self) -> Self {
            self.refill_out_bufs();
            self.refill_out_bufs();
            self
        }
        /// Returns true if the input was not exhausted (src/signal.rs:90-106).
        fn refill_out_bufs(&mut self) -> bool {
            if self.input.is_exhausted() {
                return false;
            }
            for i in 0..FRAME_SIZE {
                for (ch, samp) in self.input.next().to_float_frame().channels().enumerate() {
                    self.in_bufs[ch * FRAME_SIZE + i] = samp.to_sample::<f32>() * 32768.0;
                }
            }
            self.states.process(&mut self.out_bufs[..], &self.in_bufs[..], &mut self.vad[..], 1);
            !self.input.is_exhausted()
        }
    }

    impl<'model, S: Signal> Signal for DenoiseSignal<'model, S> {
        type Frame = <<S as Signal>::Frame as Frame>::Float;

        fn is_exhausted(&self) -> bool {
            self.out_idx >= FRAME_SIZE
        }
        fn next(&mut self) -> Self::Frame {
            if self.out_idx >= FRAME_SIZE {
                return Self::Frame::EQUILIBRIUM;
            }
            let idx = self.out_idx;
            self.out_idx += 1;
            let ret = Frame::from_fn(|ch| {
                let samp = (self.out_bufs[ch * FRAME_SIZE + idx] / 32768.0).clamp(-1.0, 1.0);
                samp.to_sample()
            });
            if self.out_idx >= FRAME_SIZE {
                if self.refill_out_bufs() {
                    self.out_idx = 0;
                }
            }
            ret
        }
    }
    #[allow(dead_code)]
    fn _frame_size_agrees() {
        let _: [(); FRAME_SIZE] = [(); DenoiseState::FRAME_SIZE];
    }
}
#[cfg(feature = "dasp")]
pub use signal::DenoiseSignal;

/// Page-locked host memory (`nnn_host_alloc`): slices of it cross the bus by DMA in `BatchDenoiser::process`, uploads and
/// downloads at the same time; ordinary slices work too, through the runtime's staging copies.
pub struct PinnedBuf {
    ptr: *mut c_float,
    len: usize,
}

impl PinnedBuf {
    pub fn new(len: usize) -> Option<PinnedBuf> {
        let ptr = unsafe { nnn_host_alloc(len * std::mem::size_of::<c_float>()) } as *mut c_float;
        if ptr.is_null() {
            None
        } else {
            unsafe { std::ptr::write_bytes(ptr, 0, len) };
            Some(PinnedBuf { ptr, len })
        }
    }
}

impl std::ops::Deref for PinnedBuf {
    type Target = [f32];
    fn deref(&self) -> &[f32] {
        unsafe { std::slice::from_raw_parts(self.ptr, self.len) }
    }
}

impl std::ops::DerefMut for PinnedBuf {
    fn deref_mut(&mut self) -> &mut [f32] {
        unsafe { std::slice::from_raw_parts_mut(self.ptr, self.len) }
    }
}

impl Drop for PinnedBuf {
    fn drop(&mut self) {
        unsafe { nnn_host_free(self.ptr as *mut c_void) }
    }
}

unsafe impl Send for PinnedBuf {}

/// All the GPUs of a node behind one object (include/nnn_node.h): the `states` vector of the reference's hosts
/// (src/nnnoiseless.rs:305-320) cut into contiguous shards, one batch and one host thread per device, no data between devices.
pub struct NodeDenoiser {
    raw: *mut RawNode,
    n: usize,
}
unsafe impl Send for NodeDenoiser {}
unsafe impl Sync for NodeDenoiser {}

impl NodeDenoiser {
    pub fn new(n_streams: usize, devices: &[i32], model: Option<&RnnModel>) -> Option<NodeDenoiser> {
        let m = model.map_or(std::ptr::null(), |m| m.0 as *const RawModel);
        let raw = unsafe { nnn_node_create(m, n_streams as c_int, devices.as_ptr(), devices.len() as c_int, std::ptr::null()) };
        if raw.is_null() {
            None
        } else {
            Some(NodeDenoiser { raw, n: n_streams })
        }
    }
    /// `input`/`output`: `[n_streams][n_frames][480]`; `vad`: `[n_frames][n_streams]`; every device works on its share at once.
    pub fn process(&mut self, output: &mut [f32], input: &[f32], vad: &mut [f32], n_frames: usize) {
        assert_eq!(input.len(), self.n * n_frames * DenoiseState::FRAME_SIZE);
        assert_eq!(output.len(), input.len());
        assert_eq!(vad.len(), self.n * n_frames);
        let rc = unsafe {
            nnn_node_process_host(
                self.raw,
                input.as_ptr(),
                output.as_mut_ptr(),
                vad.as_mut_ptr(),
                n_frames as c_int,
                n_frames * DenoiseState::FRAME_SIZE,
                DenoiseState::FRAME_SIZE,
            )
        };
        assert_eq!(rc, 0, "nnnoiseless-mi355x: backend error");
    }
    /// Buffers resident on the shards' own devices: one pointer (and optionally one `hipStream_t`) per shard; asynchronous, see `synchronize`.
    pub unsafe fn process_device(
        &mut self,
        d_out: &[*mut f32],
        d_in: &[*const f32],
        d_vad: Option<&[*mut f32]>,
        hip_streams: Option<&[*mut c_void]>,
        n_frames: usize,
        stream_stride: usize,
        frame_stride: usize,
    ) {
        let n = nnn_node_num_shards(self.raw) as usize;
        assert!(d_in.len() == n && d_out.len() == n, "one table entry per shard");
        assert!(d_vad.map_or(true, |v| v.len() == n) && hip_streams.map_or(true, |v| v.len() == n), "one table entry per shard");
        let rc = nnn_node_process_device_streams(
            self.raw,
            d_in.as_ptr(),
            d_out.as_ptr(),
            d_vad.map_or(std::ptr::null(), |v| v.as_ptr()),
            hip_streams.map_or(std::ptr::null(), |v| v.as_ptr()),
            n as c_int,
            n_frames as c_int,
            stream_stride,
            frame_stride,
        );
        assert_eq!(rc, 0, "nnnoiseless-mi355x: backend error");
    }
    pub fn synchronize(&mut self) {
        assert_eq!(unsafe { nnn_node_synchronize(self.raw) }, 0, "nnnoiseless-mi355x: backend error");
    }
    /// The CPUs shard `i`'s host thread is pinned to (its device's local CPUs); empty when not pinned.
    pub fn shard_cpus(&self, i: usize) -> String {
        unsafe { std::ffi::CStr::from_ptr(nnn_node_shard_cpus(self.raw, i as c_int)).to_string_lossy().into_owned() }
    }
    /// Also clears the failed state a call leaves behind when one shard fails (the others have advanced).
    pub fn reset(&mut self) {
        unsafe { nnn_node_reset(self.raw) };
    }
}
impl Drop for NodeDenoiser {
    fn drop(&mut self) {
        unsafe { nnn_node_destroy(self.raw) }
    }
}
