"""ctypes binding of the C ABI in include/nnn_batch.h and include/rnnoise.h."""
import ctypes as C
import os

import numpy as np

FRAME_SIZE = 480

TAPS = ["filtered", "xlp", "ac", "lpc2", "xcorr1", "best1", "xcorr2c", "pitch_search", "pitch", "pitch_gain",
        "X", "P", "ex", "ep", "exp", "features", "silence", "g_raw", "g", "vad", "branch"]

# every symbol the two headers declare (tests check that the built library exports all of them)
BATCH_SYMBOLS = [
    "nnn_model_from_bytes", "nnn_model_default", "nnn_model_free", "nnn_model_clone", "nnn_model_shape",
    "nnn_convert_rnnoise_text", "nnn_model_from_rnnoise_text",
    "nnn_batch_create", "nnn_batch_create_grouped", "nnn_batch_destroy", "nnn_batch_num_streams", "nnn_batch_reset",
    "nnn_batch_process_device", "nnn_batch_process_host", "nnn_batch_process_pcm_device", "nnn_batch_process_pcm_host",
    "nnn_batch_synchronize", "nnn_batch_clone", "nnn_batch_state_bytes", "nnn_batch_save_state", "nnn_batch_load_state",
    "nnn_batch_set_taps", "nnn_batch_set_schedule", "nnn_batch_set_inputs_ready", "nnn_debug_activations",
    "nnn_tap_info", "nnn_batch_read_tap", "nnn_batch_set_profiling", "nnn_batch_num_kernels",
    "nnn_batch_kernel_name", "nnn_batch_read_kernel_times", "nnn_batch_set_graph", "nnn_batch_set_pipeline", "nnn_batch_read_stamps",
    "nnn_host_alloc", "nnn_host_free", "nnn_last_error", "nnn_batch_fault", "nnn_batch_debug_withhold_flag", "nnn_batch_debug_schedule", "nnn_batch_debug_host_plan", "nnn_batch_set_frame_log",
    "nnn_batch_create_opts", "nnn_batch_max_group_frames", "nnn_batch_device_bytes", "nnn_batch_set_back_end", "nnn_device_local_cpulist",
    "nnn_batch_reset_streams", "nnn_batch_export_streams", "nnn_batch_import_streams", "nnn_batch_export_streams_device",
    "nnn_batch_import_streams_device", "nnn_batch_hold_streams", "nnn_batch_resume_streams", "nnn_batch_num_held", "nnn_batch_held_mask",
    "nnn_batch_analyze_device", "nnn_batch_synthesize_device", "nnn_batch_analyze_host", "nnn_batch_synthesize_host", "nnn_batch_pending_frames",
    "nnn_batch_vad_device", "nnn_batch_vad_host", "nnn_batch_network_device", "nnn_batch_network_host",
    "nnn_batch_set_gain_floor", "nnn_batch_get_gain_floor", "nnn_batch_num_floored",
    "nnn_batch_set_channel_link", "nnn_batch_get_channel_link",
]
TRAIN_SYMBOLS = [
    "nnn_train_create", "nnn_train_destroy", "nnn_train_reset", "nnn_train_process_device", "nnn_train_process_host",
]
RESAMPLE_SYMBOLS = [
    "nnn_resampler_create", "nnn_resampler_destroy", "nnn_resampler_reset", "nnn_resampler_max_output",
    "nnn_resampler_process_device", "nnn_resampler_process_host",
]
# include/nnn_rate.h (the rate adapter; a list of its own: the adapter is an object beside the batch, not part of it)
RATE_SYMBOLS = [
    "nnn_rate_create", "nnn_rate_destroy", "nnn_rate_reset", "nnn_rate_reset_streams", "nnn_rate_max_output", "nnn_rate_max_frames",
    "nnn_rate_carried", "nnn_rate_process_device", "nnn_rate_process_host", "nnn_rate_debug_tables",
]
# include/nnn_pack.h (the file packer; a list of its own for the same reason)
PACK_SYMBOLS = [
    "nnn_pack_create", "nnn_pack_destroy", "nnn_pack_plan", "nnn_pack_run_device", "nnn_pack_run_host", "nnn_pack_last_summary",
    "nnn_pack_debug_kernels",
]
# include/nnn_sim.h (the noise simulator of the training-data generator; an object beside nnn_train)
SIM_SYMBOLS = [
    "nnn_sim_create", "nnn_sim_destroy", "nnn_sim_load", "nnn_sim_adopt_device", "nnn_sim_set_params", "nnn_sim_get_params", "nnn_sim_reset",
    "nnn_sim_process_device", "nnn_sim_process_host", "nnn_sim_signals_device", "nnn_sim_signals_host", "nnn_sim_fault", "nnn_sim_debug_kernel",
]
# include/nnn_fit.h (the network trainer: rows in, a .rnn model out)
FIT_SYMBOLS = [
    "nnn_fit_create", "nnn_fit_destroy", "nnn_fit_get", "nnn_fit_set", "nnn_fit_get_step", "nnn_fit_set_step", "nnn_fit_get_settings",
    "nnn_fit_set_settings", "nnn_fit_export_rnn", "nnn_fit_forward_device", "nnn_fit_loss_device", "nnn_fit_grad_device", "nnn_fit_step",
    "nnn_fit_losses", "nnn_fit_forward_host", "nnn_fit_loss_host", "nnn_fit_grad_host", "nnn_fit_debug_recurrence",
]
# include/nnn_score.h (the scorer: sums between a reference and a test signal; an object beside the simulator and the trainer)
SCORE_SYMBOLS = [
    "nnn_score_create", "nnn_score_destroy", "nnn_score_set_delay", "nnn_score_get_delay", "nnn_score_reset", "nnn_score_accumulate_device",
    "nnn_score_accumulate_host", "nnn_score_totals", "nnn_score_totals_device",
]
SCORE_MAX_DELAY, SCORE_SUMS = 960, 4
# include/nnn_gate.h (the VAD gate: threshold, grace and look-back per stream behind the denoiser; an object beside the batch)
GATE_SYMBOLS = [
    "nnn_gate_create", "nnn_gate_destroy", "nnn_gate_set_params", "nnn_gate_get_params", "nnn_gate_reset", "nnn_gate_apply_device",
    "nnn_gate_apply_pcm_device", "nnn_gate_apply_host", "nnn_gate_state_bytes", "nnn_gate_export_streams", "nnn_gate_import_streams",
]
GATE_MAX_LOOKBACK, GATE_MAX_GRACE, GATE_NEVER = 8, 6000, 0x7fffffff
GATE_STATE_BYTES, GATE_STATE_VERSION, GATE_STATE_MAGIC = 48 + 8 * 480 * 4, 1, 0x3147564E
# struct nnn_gate_params as a numpy dtype: what VadGate.params returns
GATE_PARAMS_DTYPE = np.dtype([("threshold", "<f4"), ("grace", "<i4"), ("lookback", "<i4"), ("level", "<f4")])
# a stream's record (NNN_GATE_STATE_BYTES): the header's fields and the history rows
GATE_STATE_DTYPE = np.dtype([("magic", "<u4"), ("version", "<u4"), ("size", "<u4"), ("threshold", "<f4"), ("grace", "<i4"), ("lookback", "<i4"),
                             ("level", "<f4"), ("since", "<i4"), ("was_open", "<u4"), ("zero", "<u4", 3), ("history", "<f4", (8, 480))])
# include/nnn_mix.h (the conference mixer: per-room mix-minus behind the gate; an object beside the batch)
MIX_SYMBOLS = [
    "nnn_mix_create", "nnn_mix_destroy", "nnn_mix_set_rooms", "nnn_mix_get_rooms", "nnn_mix_set_gains", "nnn_mix_get_gains", "nnn_mix_reset",
    "nnn_mix_apply_device", "nnn_mix_apply_pcm_device", "nnn_mix_apply_host",
]
MIX_MAX_GAIN, MIX_TILE, MIX_REG_TALKERS = 16, 32, 8
# include/nnn_pick.h (the talker picker: the k loudest open gates of a room, between the gate and the mixer; an object beside the batch)
PICK_SYMBOLS = [
    "nnn_pick_create", "nnn_pick_destroy", "nnn_pick_set_rooms", "nnn_pick_get_rooms", "nnn_pick_set_pinned", "nnn_pick_get_pinned",
    "nnn_pick_set_policy", "nnn_pick_get_policy", "nnn_pick_reset", "nnn_pick_select_device", "nnn_pick_select_pcm_device", "nnn_pick_select_host",
]
PICK_MAX_K, PICK_MAX_STICK, PICK_SEG_ROOM, PICK_WAVE_ROOM = 8, 16, 8, 64
FIT_PARAMS, FIT_RNN_BYTES, FIT_TILE = 87503, 87521, 4
FIT_SEL_PARAMS, FIT_SEL_GRAD, FIT_SEL_ADAM_M, FIT_SEL_ADAM_V = 0, 1, 2, 3
# the fifteen tensors of the parameter vector (NNN_FIT_OFF_*): name -> (offset, shape)
FIT_TENSORS = {
    "input_dense.W": (0, (42, 24)), "input_dense.b": (1008, (24,)),
    "vad_gru.W": (1032, (24, 72)), "vad_gru.U": (2760, (24, 72)), "vad_gru.b": (4488, (72,)),
    "noise_gru.W": (4560, (90, 144)), "noise_gru.U": (17520, (48, 144)), "noise_gru.b": (24432, (144,)),
    "denoise_gru.W": (24576, (114, 288)), "denoise_gru.U": (57408, (96, 288)), "denoise_gru.b": (85056, (288,)),
    "denoise_output.W": (85344, (96, 22)), "denoise_output.b": (87456, (22,)),
    "vad_output.W": (87478, (24, 1)), "vad_output.b": (87502, (1,)),
}
NODE_SYMBOLS = [
    "nnn_node_create", "nnn_node_destroy", "nnn_node_num_streams", "nnn_node_num_shards", "nnn_node_shard", "nnn_node_batch", "nnn_node_reset",
    "nnn_node_process_host", "nnn_node_process_pcm_host", "nnn_node_process_device", "nnn_node_process_device_streams", "nnn_node_synchronize",
    "nnn_node_fault", "nnn_node_shard_cpus", "nnn_node_reset_streams", "nnn_node_export_streams", "nnn_node_import_streams",
    "nnn_node_hold_streams", "nnn_node_resume_streams", "nnn_node_num_held",
    "nnn_node_set_gain_floor", "nnn_node_get_gain_floor", "nnn_node_num_floored",
    "nnn_node_set_channel_link", "nnn_node_get_channel_link",
]
RNNOISE_SYMBOLS = [
    "rnnoise_get_frame_size", "rnnoise_get_size", "rnnoise_init", "rnnoise_create", "rnnoise_destroy",
    "rnnoise_process_frame", "rnnoise_model_from_file", "rnnoise_model_free",
]


PCM_F32, PCM_I16, PCM_F32_UNIT = 0, 1, 2
PACK_I24, PACK_I32, PACK_F32_WAV = 16, 17, 18   # enum nnn_pack_format (include/nnn_pack.h): the packer's further INPUT formats
PACK_ELEM_BYTES = {PCM_F32: 4, PCM_I16: 2, PACK_I24: 3, PACK_I32: 4, PACK_F32_WAV: 4}
LINK_OFF, LINK_MAX, LINK_MIN = 0, 1, 2   # enum nnn_link_mode
LINK_MODES = {"off": LINK_OFF, "max": LINK_MAX, "min": LINK_MIN}

# per-stream state records (include/nnn_batch.h NNN_STREAM_STATE_*): byte offsets of the fields
STREAM_STATE_BYTES = 11232
STREAM_STATE_VERSION = 1
STREAM_STATE_MAGIC = 0x3153534E
STREAM_STATE_FIELDS = {   # name: (byte offset, numpy dtype, count)
    "magic": (0, np.uint32, 1), "version": (4, np.uint32, 1), "size": (8, np.uint32, 1), "gru_sizes": (12, np.int32, 3),
    "mem_id": (24, np.int32, 1), "last_period": (28, np.int32, 1), "last_gain": (32, np.float32, 1), "mem_hp_x": (36, np.float32, 2),
    "input_mem": (64, np.float32, 1728), "synthesis_mem": (6976, np.float32, 480), "cepstral_mem": (8896, np.float32, 176),
    "lastg": (9600, np.float32, 22), "vad_gru": (9696, np.float32, 128), "noise_gru": (10208, np.float32, 128),
    "denoise_gru": (10720, np.float32, 128),
}


def stream_state_field(records, name):
    """A field of one record ([STREAM_STATE_BYTES] uint8) or of a stack of them ([n, STREAM_STATE_BYTES]) as numbers: [..., count]."""
    off, dt, cnt = STREAM_STATE_FIELDS[name]
    r = np.ascontiguousarray(records, dtype=np.uint8)
    a = r[..., off:off + cnt * np.dtype(dt).itemsize].view(dt)
    return a.reshape(r.shape[:-1] + (cnt,))
PCM_DTYPE = {PCM_F32: np.float32, PCM_I16: np.int16, PCM_F32_UNIT: np.float32}


class PcmLayout(C.Structure):
    """struct nnn_pcm_layout (include/nnn_batch.h)."""
    _fields_ = [("format", C.c_int), ("channels", C.c_int), ("discard_first", C.c_int), ("reserved", C.c_int),
                ("group_stride", C.c_size_t), ("frame_stride", C.c_size_t)]


class PackFile(C.Structure):
    """struct nnn_pack_file (include/nnn_pack.h)."""
    _fields_ = [("in_off", C.c_uint64), ("n_frames_samples", C.c_uint64), ("out_off", C.c_uint64), ("vad_off", C.c_uint64)]


class SimParams(C.Structure):
    """struct nnn_sim_params (include/nnn_sim.h)."""
    _fields_ = [("signal_gain", C.c_float), ("noise_gain", C.c_float), ("sig_a", C.c_float * 2), ("sig_b", C.c_float * 2),
                ("noise_a", C.c_float * 2), ("noise_b", C.c_float * 2), ("band_lp", C.c_int32)]


# the same record as a numpy dtype: what training.NoiseSimulator.params returns and set_params takes
SIM_PARAMS_DTYPE = np.dtype([("signal_gain", "<f4"), ("noise_gain", "<f4"), ("sig_a", "<f4", 2), ("sig_b", "<f4", 2),
                             ("noise_a", "<f4", 2), ("noise_b", "<f4", 2), ("band_lp", "<i4")])


class FitSettings(C.Structure):
    """struct nnn_fit_settings (include/nnn_fit.h)."""
    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("epsilon", C.c_float), ("reg", C.c_float), ("clip", C.c_float)]


class FitRows(C.Structure):
    """struct nnn_fit_rows (include/nnn_fit.h)."""
    _fields_ = [("rows", C.c_void_p), ("frame_stride", C.c_size_t), ("seq_stride", C.c_size_t), ("w", C.c_void_p),
                ("w_frame_stride", C.c_size_t), ("w_seq_stride", C.c_size_t), ("n_seq", C.c_int), ("window", C.c_int)]


class BatchOpts(C.Structure):
    """struct nnn_batch_opts (include/nnn_batch.h)."""
    _fields_ = [("max_group_frames", C.c_int), ("reserved", C.c_int * 7)]


class Library:
    """A loaded build of the backend.  The package default is the hipcc-built gfx950 library."""

    def __init__(self, path):
        if not os.path.exists(path):
            raise RuntimeError(
                f"nnnoiseless_amd: HIP library not found at {path}. Build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc); there is no CPU fallback.")
        self.path = path
        L = self.L = C.CDLL(path)
        vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
        L.nnn_model_from_bytes.restype = vp
        L.nnn_model_from_bytes.argtypes = [C.c_char_p, sz]
        L.nnn_model_default.restype = vp
        L.nnn_model_free.argtypes = [vp]
        L.nnn_model_clone.restype = vp
        L.nnn_model_clone.argtypes = [vp]
        L.nnn_model_shape.argtypes = [vp, C.POINTER(C.c_int32)]
        L.nnn_convert_rnnoise_text.restype = C.c_long
        L.nnn_convert_rnnoise_text.argtypes = [C.c_char_p, sz, vp, sz]
        L.nnn_model_from_rnnoise_text.restype = vp
        L.nnn_model_from_rnnoise_text.argtypes = [C.c_char_p, sz]
        L.nnn_batch_create_grouped.restype = vp
        L.nnn_batch_create_grouped.argtypes = [C.POINTER(vp), C.POINTER(i32), i32, i32]
        L.nnn_batch_create.restype = vp
        L.nnn_batch_create.argtypes = [vp, i32, i32]
        L.nnn_batch_destroy.argtypes = [vp]
        L.nnn_batch_num_streams.argtypes = [vp]
        L.nnn_batch_reset.argtypes = [vp]
        L.nnn_batch_process_device.argtypes = [vp, vp, vp, vp, i32, sz, sz, vp]
        L.nnn_batch_process_host.argtypes = [vp, vp, vp, vp, i32, sz, sz]
        L.nnn_batch_process_pcm_device.argtypes = [vp, vp, vp, vp, i32, C.POINTER(PcmLayout), vp]
        L.nnn_batch_process_pcm_host.argtypes = [vp, vp, vp, vp, i32, C.POINTER(PcmLayout)]
        L.nnn_batch_synchronize.argtypes = [vp]
        L.nnn_host_alloc.restype = vp
        L.nnn_host_alloc.argtypes = [sz]
        L.nnn_host_free.restype = None
        L.nnn_host_free.argtypes = [vp]
        L.nnn_tap_info.argtypes = [i32, C.POINTER(i32), C.POINTER(i32)]
        L.nnn_batch_read_tap.argtypes = [vp, i32, vp, sz]
        L.nnn_batch_set_profiling.argtypes = [vp, i32]
        L.nnn_batch_kernel_name.restype = C.c_char_p
        L.nnn_batch_kernel_name.argtypes = [i32]
        L.nnn_batch_read_kernel_times.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), i32]
        L.nnn_batch_set_graph.argtypes = [vp, i32]
        L.nnn_batch_clone.restype = vp
        L.nnn_batch_clone.argtypes = [vp]
        L.nnn_batch_state_bytes.restype = sz
        L.nnn_batch_state_bytes.argtypes = [vp]
        L.nnn_batch_save_state.argtypes = [vp, vp, sz]
        L.nnn_batch_load_state.argtypes = [vp, vp, sz]
        L.nnn_batch_set_taps.argtypes = [vp, i32]
        L.nnn_batch_set_schedule.argtypes = [vp, i32, i32]
        L.nnn_debug_activations.argtypes = [i32, i32, vp, vp, i32]
        L.nnn_batch_set_pipeline.argtypes = [vp, i32]
        L.nnn_batch_set_inputs_ready.argtypes = [vp, i32]
        for name, at in (("nnn_batch_set_frame_log", [vp, vp, sz]), ("nnn_batch_fault", [vp]), ("nnn_batch_debug_withhold_flag", [vp, i32]),
                         ("nnn_batch_debug_schedule", [vp, i32, C.POINTER(C.c_int32), sz]),
                         ("nnn_batch_debug_host_plan", [vp, i32, C.POINTER(PcmLayout), i32, C.POINTER(C.c_int64)]),
                         ("nnn_batch_create_opts", [C.POINTER(vp), C.POINTER(i32), i32, i32, C.POINTER(BatchOpts)]),
                         ("nnn_batch_max_group_frames", [vp]), ("nnn_batch_device_bytes", [vp]), ("nnn_batch_set_back_end", [vp, i32])):
            if hasattr(L, name):   # (experimental builds of older sources, loaded through NNN_LIBRARY, lack the newest entry points)
                getattr(L, name).argtypes = at
        if hasattr(L, "nnn_batch_create_opts"):
            L.nnn_batch_create_opts.restype = vp
            L.nnn_batch_device_bytes.restype = sz
        if hasattr(L, "nnn_batch_reset_streams"):
            ip = C.POINTER(i32)
            L.nnn_batch_reset_streams.argtypes = [vp, ip, i32]
            L.nnn_batch_export_streams.argtypes = [vp, ip, i32, vp, sz]
            L.nnn_batch_import_streams.argtypes = [vp, ip, i32, vp, sz]
            L.nnn_batch_export_streams_device.argtypes = [vp, ip, i32, vp, vp]
            L.nnn_batch_import_streams_device.argtypes = [vp, ip, i32, vp, vp]
        if hasattr(L, "nnn_batch_hold_streams"):
            ip = C.POINTER(i32)
            L.nnn_batch_hold_streams.argtypes = [vp, ip, i32]
            L.nnn_batch_resume_streams.argtypes = [vp, ip, i32]
            L.nnn_batch_num_held.argtypes = [vp]
            L.nnn_batch_held_mask.argtypes = [vp, vp, sz]
        if hasattr(L, "nnn_batch_analyze_device"):
            lp = C.POINTER(PcmLayout)
            L.nnn_batch_analyze_device.argtypes = [vp, vp, vp, vp, i32, lp, vp]
            L.nnn_batch_synthesize_device.argtypes = [vp, vp, vp, vp, i32, lp, vp]
            L.nnn_batch_analyze_host.argtypes = [vp, vp, vp, vp, i32, lp]
            L.nnn_batch_synthesize_host.argtypes = [vp, vp, vp, vp, i32, lp]
            L.nnn_batch_pending_frames.argtypes = [vp]
        if hasattr(L, "nnn_batch_vad_device"):
            L.nnn_batch_vad_device.argtypes = [vp, vp, vp, i32, C.POINTER(PcmLayout), vp]
            L.nnn_batch_vad_host.argtypes = [vp, vp, vp, i32, C.POINTER(PcmLayout)]
        if hasattr(L, "nnn_batch_network_device"):
            L.nnn_batch_network_device.argtypes = [vp, vp, vp, vp, vp, i32, vp]
            L.nnn_batch_network_host.argtypes = [vp, vp, vp, vp, vp, i32]
        if hasattr(L, "nnn_batch_set_gain_floor"):
            ip, fp = C.POINTER(i32), C.POINTER(C.c_float)
            L.nnn_batch_set_gain_floor.argtypes = [vp, ip, i32, fp, i32]
            L.nnn_batch_get_gain_floor.argtypes = [vp, ip, i32, fp]
            L.nnn_batch_num_floored.argtypes = [vp]
        for name in ("nnn_batch_set_channel_link", "nnn_node_set_channel_link"):
            if hasattr(L, name):
                getattr(L, name).argtypes = [vp, i32, i32]
                getattr(L, name.replace("_set_", "_get_")).argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
        if hasattr(L, "nnn_node_set_gain_floor"):
            ip, fp = C.POINTER(i32), C.POINTER(C.c_float)
            L.nnn_node_set_gain_floor.argtypes = [vp, ip, i32, fp, i32]
            L.nnn_node_get_gain_floor.argtypes = [vp, ip, i32, fp]
            L.nnn_node_num_floored.argtypes = [vp]
        if hasattr(L, "nnn_node_hold_streams"):
            ip = C.POINTER(i32)
            L.nnn_node_hold_streams.argtypes = [vp, ip, i32]
            L.nnn_node_resume_streams.argtypes = [vp, ip, i32]
            L.nnn_node_num_held.argtypes = [vp]
        if hasattr(L, "nnn_node_reset_streams"):
            ip = C.POINTER(i32)
            L.nnn_node_reset_streams.argtypes = [vp, ip, i32]
            L.nnn_node_export_streams.argtypes = [vp, ip, i32, vp, sz]
            L.nnn_node_import_streams.argtypes = [vp, ip, i32, vp, sz]
        if hasattr(L, "nnn_node_create"):
            L.nnn_node_create.restype = vp
            L.nnn_node_create.argtypes = [vp, i32, C.POINTER(i32), i32, C.POINTER(BatchOpts)]
            L.nnn_node_destroy.argtypes = [vp]
            L.nnn_node_num_streams.argtypes = [vp]
            L.nnn_node_num_shards.argtypes = [vp]
            L.nnn_node_shard.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
            L.nnn_node_batch.restype = vp
            L.nnn_node_batch.argtypes = [vp, i32]
            L.nnn_node_reset.argtypes = [vp]
            L.nnn_node_process_host.argtypes = [vp, vp, vp, vp, i32, sz, sz]
            L.nnn_node_process_pcm_host.argtypes = [vp, vp, vp, vp, i32, C.POINTER(PcmLayout)]
            L.nnn_node_process_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i32, sz, sz]
            L.nnn_node_process_device_streams.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i32, i32, sz, sz]
            L.nnn_node_shard_cpus.restype = C.c_char_p
            L.nnn_node_shard_cpus.argtypes = [vp, i32]
            L.nnn_node_synchronize.argtypes = [vp]
            L.nnn_node_fault.argtypes = [vp]
        L.nnn_train_create.restype = vp
        L.nnn_train_create.argtypes = [i32, i32]
        L.nnn_train_destroy.argtypes = [vp]
        L.nnn_train_reset.argtypes = [vp]
        L.nnn_train_process_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, sz, sz, vp]
        L.nnn_train_process_host.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32]
        L.nnn_resampler_create.restype = vp
        L.nnn_resampler_create.argtypes = [i32, C.c_double, i32]
        L.nnn_resampler_destroy.argtypes = [vp]
        L.nnn_resampler_reset.argtypes = [vp]
        L.nnn_resampler_max_output.restype = C.c_long
        L.nnn_resampler_max_output.argtypes = [vp, C.c_long]
        L.nnn_resampler_process_device.argtypes = [vp, vp, C.c_long, sz, vp, C.c_long, sz, C.POINTER(C.c_long), vp]
        L.nnn_resampler_process_host.argtypes = [vp, vp, C.c_long, vp, C.c_long, C.POINTER(C.c_long)]
        if hasattr(L, "nnn_rate_create"):
            lp = C.POINTER(C.c_long)
            L.nnn_rate_create.restype = vp
            L.nnn_rate_create.argtypes = [vp, C.c_double, C.c_long]
            L.nnn_rate_destroy.restype = None
            L.nnn_rate_destroy.argtypes = [vp]
            L.nnn_rate_reset.argtypes = [vp]
            L.nnn_rate_reset_streams.argtypes = [vp, C.POINTER(i32), i32]
            L.nnn_rate_max_output.restype = C.c_long
            L.nnn_rate_max_output.argtypes = [vp, C.c_long]
            L.nnn_rate_max_frames.argtypes = [vp, C.c_long]
            L.nnn_rate_carried.restype = C.c_long
            L.nnn_rate_carried.argtypes = [vp]
            L.nnn_rate_process_device.argtypes = [vp, vp, C.c_long, sz, vp, C.c_long, sz, lp, vp, i32, C.POINTER(i32), i32, vp]
            L.nnn_rate_process_host.argtypes = [vp, vp, C.c_long, vp, C.c_long, lp, vp, i32, C.POINTER(i32), i32]
            L.nnn_rate_debug_tables.argtypes = [vp, lp, C.POINTER(C.c_double)]
        if hasattr(L, "nnn_pack_create"):
            u64, fp_ = C.c_uint64, C.POINTER(PackFile)
            L.nnn_pack_create.restype = vp
            L.nnn_pack_create.argtypes = [vp, i32, i32]
            L.nnn_pack_destroy.restype = None
            L.nnn_pack_destroy.argtypes = [vp]
            L.nnn_pack_plan.argtypes = [i32, i32, C.POINTER(u64), i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
            L.nnn_pack_run_device.argtypes = [vp, vp, u64, i32, vp, u64, i32, vp, u64, fp_, i32, vp]
            L.nnn_pack_run_host.argtypes = [vp, vp, u64, i32, vp, u64, i32, vp, u64, fp_, i32]
            L.nnn_pack_last_summary.argtypes = [vp, C.POINTER(C.c_int64)]
            L.nnn_pack_debug_kernels.argtypes = [vp, i32, vp, i32, vp, i32, i32, i32, vp]
        if hasattr(L, "nnn_sim_create"):
            u64, ip = C.c_uint64, C.POINTER(i32)
            L.nnn_sim_create.restype = vp
            L.nnn_sim_create.argtypes = [vp]
            L.nnn_sim_destroy.restype = None
            L.nnn_sim_destroy.argtypes = [vp]
            L.nnn_sim_load.argtypes = [vp, i32, vp, u64]
            L.nnn_sim_adopt_device.argtypes = [vp, i32, vp, u64]
            L.nnn_sim_set_params.argtypes = [vp, ip, i32, vp]
            L.nnn_sim_get_params.argtypes = [vp, ip, i32, vp]
            L.nnn_sim_reset.argtypes = [vp]
            L.nnn_sim_process_device.argtypes = [vp, vp, vp, vp, i32, vp]
            L.nnn_sim_process_host.argtypes = [vp, vp, vp, vp, i32]
            L.nnn_sim_signals_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i32, sz, sz, vp]
            L.nnn_sim_signals_host.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i32]
            L.nnn_sim_fault.argtypes = [vp]
            L.nnn_sim_debug_kernel.argtypes = [vp, vp, vp, i32, i32, vp]
        if hasattr(L, "nnn_fit_create"):
            rp, fp = C.POINTER(FitRows), C.POINTER(C.c_float)
            L.nnn_fit_create.restype = vp
            L.nnn_fit_create.argtypes = [C.c_char_p, sz, i32, i32, i32]
            L.nnn_fit_destroy.restype = None
            L.nnn_fit_destroy.argtypes = [vp]
            L.nnn_fit_get.argtypes = [vp, i32, vp]
            L.nnn_fit_set.argtypes = [vp, i32, vp]
            L.nnn_fit_get_step.argtypes = [vp, C.POINTER(C.c_int64)]
            L.nnn_fit_set_step.argtypes = [vp, C.c_int64]
            L.nnn_fit_get_settings.argtypes = [vp, C.POINTER(FitSettings)]
            L.nnn_fit_set_settings.argtypes = [vp, C.POINTER(FitSettings)]
            L.nnn_fit_export_rnn.argtypes = [vp, vp, sz]
            L.nnn_fit_forward_device.argtypes = [vp, rp, vp, vp, vp]
            L.nnn_fit_loss_device.argtypes = [vp, rp, vp]
            L.nnn_fit_grad_device.argtypes = [vp, rp, vp]
            L.nnn_fit_step.argtypes = [vp, vp]
            L.nnn_fit_losses.argtypes = [vp, fp]
            L.nnn_fit_forward_host.argtypes = [vp, vp, i32, i32, vp, vp]
            L.nnn_fit_loss_host.argtypes = [vp, vp, vp, i32, i32]
            L.nnn_fit_grad_host.argtypes = [vp, vp, vp, i32, i32]
            L.nnn_fit_debug_recurrence.argtypes = [vp, i32, i32, i32, i32, i32, vp]
        if hasattr(L, "nnn_score_create"):
            ip = C.POINTER(i32)
            L.nnn_score_create.restype = vp
            L.nnn_score_create.argtypes = [i32, i32, i32]
            L.nnn_score_destroy.restype = None
            L.nnn_score_destroy.argtypes = [vp]
            L.nnn_score_set_delay.argtypes = [vp, ip, i32, vp]
            L.nnn_score_get_delay.argtypes = [vp, ip, i32, vp]
            L.nnn_score_reset.argtypes = [vp, ip, i32]
            L.nnn_score_accumulate_device.argtypes = [vp, vp, vp, vp, vp, i32, sz, sz, vp]
            L.nnn_score_accumulate_host.argtypes = [vp, vp, vp, vp, vp, i32]
            L.nnn_score_totals.argtypes = [vp, vp, vp]
            L.nnn_score_totals_device.argtypes = [vp, vp, vp, vp]
        if hasattr(L, "nnn_gate_create"):
            ip = C.POINTER(i32)
            L.nnn_gate_create.restype = vp
            L.nnn_gate_create.argtypes = [i32, i32, i32]
            L.nnn_gate_destroy.restype = None
            L.nnn_gate_destroy.argtypes = [vp]
            L.nnn_gate_set_params.argtypes = [vp, ip, i32, vp]
            L.nnn_gate_get_params.argtypes = [vp, ip, i32, vp]
            L.nnn_gate_reset.argtypes = [vp, ip, i32]
            L.nnn_gate_apply_device.argtypes = [vp, vp, vp, vp, vp, vp, i32, sz, sz, vp]
            L.nnn_gate_apply_pcm_device.argtypes = [vp, vp, vp, vp, vp, vp, i32, C.POINTER(PcmLayout), vp]
            L.nnn_gate_apply_host.argtypes = [vp, vp, vp, vp, vp, vp, i32]
            L.nnn_gate_state_bytes.restype = sz
            L.nnn_gate_state_bytes.argtypes = [vp]
            L.nnn_gate_export_streams.argtypes = [vp, ip, i32, vp, sz]
            L.nnn_gate_import_streams.argtypes = [vp, ip, i32, vp, sz]
        if hasattr(L, "nnn_mix_create"):
            ip, lp = C.POINTER(i32), C.POINTER(PcmLayout)
            L.nnn_mix_create.restype = vp
            L.nnn_mix_create.argtypes = [i32, i32]
            L.nnn_mix_destroy.restype = None
            L.nnn_mix_destroy.argtypes = [vp]
            L.nnn_mix_set_rooms.argtypes = [vp, ip, i32, vp]
            L.nnn_mix_get_rooms.argtypes = [vp, ip, i32, vp]
            L.nnn_mix_set_gains.argtypes = [vp, ip, i32, vp]
            L.nnn_mix_get_gains.argtypes = [vp, ip, i32, vp]
            L.nnn_mix_reset.argtypes = [vp, ip, i32]
            L.nnn_mix_apply_device.argtypes = [vp, vp, vp, vp, vp, vp, i32, sz, sz, sz, sz, vp]
            L.nnn_mix_apply_pcm_device.argtypes = [vp, vp, vp, vp, vp, vp, i32, lp, lp, vp]
            L.nnn_mix_apply_host.argtypes = [vp, vp, vp, vp, vp, vp, i32]
        if hasattr(L, "nnn_pick_create"):
            ip, lp, fp = C.POINTER(i32), C.POINTER(PcmLayout), C.POINTER(C.c_float)
            L.nnn_pick_create.restype = vp
            L.nnn_pick_create.argtypes = [i32, i32]
            L.nnn_pick_destroy.restype = None
            L.nnn_pick_destroy.argtypes = [vp]
            L.nnn_pick_set_rooms.argtypes = [vp, ip, i32, vp]
            L.nnn_pick_get_rooms.argtypes = [vp, ip, i32, vp]
            L.nnn_pick_set_pinned.argtypes = [vp, ip, i32, vp]
            L.nnn_pick_get_pinned.argtypes = [vp, ip, i32, vp]
            L.nnn_pick_set_policy.argtypes = [vp, i32, C.c_float, C.c_float]
            L.nnn_pick_get_policy.argtypes = [vp, ip, fp, fp]
            L.nnn_pick_reset.argtypes = [vp, ip, i32]
            L.nnn_pick_select_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, sz, sz, vp]
            L.nnn_pick_select_pcm_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, lp, vp]
            L.nnn_pick_select_host.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32]
        L.nnn_last_error.restype = C.c_char_p
        L.rnnoise_create.restype = vp
        L.rnnoise_create.argtypes = [vp]
        L.rnnoise_destroy.argtypes = [vp]
        L.rnnoise_process_frame.restype = C.c_float
        L.rnnoise_process_frame.argtypes = [vp, vp, vp]
        L.rnnoise_model_free.argtypes = [vp]

    def error(self):
        return self.L.nnn_last_error().decode()

    def check(self, rc):
        if rc != 0:
            raise RuntimeError("nnnoiseless_amd: " + self.error())


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def as_f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def stream_list(idx):
    """A stream index list as the int32 array the C ABI takes (host memory) and a pointer to it."""
    a = np.ascontiguousarray(np.asarray(idx, dtype=np.int64).reshape(-1))
    if a.size and (a.min() < -2**31 or a.max() >= 2**31):
        raise ValueError("stream index out of int32 range")
    a = a.astype(np.int32)
    return a, a.ctypes.data_as(C.POINTER(C.c_int))


def stream_records(records, n):
    """n records as one C-contiguous uint8 block [n, STREAM_STATE_BYTES]."""
    r = np.ascontiguousarray(records, dtype=np.uint8)
    if r.size != n * STREAM_STATE_BYTES:
        raise ValueError(f"need {n} records of {STREAM_STATE_BYTES} bytes, got {r.size} bytes")
    return r.reshape(n, STREAM_STATE_BYTES)


def gain_floors(floors, n):
    """Floors for n listed streams as the float32 block the C ABI takes and its `bands`: a scalar (every listed stream, all bands), [n] (one
    value per stream, all its bands) -> bands 1; [n, 22] -> bands 22."""
    f = np.asarray(floors, dtype=np.float32)
    if f.ndim == 0:
        f = np.full(n, f, np.float32)
    if f.shape == (n,):
        return np.ascontiguousarray(f), 1
    if f.shape == (n, 22):
        return np.ascontiguousarray(f), 22
    raise ValueError(f"floors must be a scalar, [{n}] or [{n}, 22], got shape {f.shape}")


def link_mode(mode):
    """enum nnn_link_mode of "off" / "max" / "min" or of the number itself."""
    if isinstance(mode, str):
        if mode not in LINK_MODES:
            raise ValueError(f"link mode must be one of {sorted(LINK_MODES)}, got {mode!r}")
        return LINK_MODES[mode]
    return int(mode)


def link_mode_name(mode):
    return {v: k for k, v in LINK_MODES.items()}[int(mode)]
