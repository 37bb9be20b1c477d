"""ctypes binding of libacm_hip.so (include/acm_hip.h + include/libacm.h).

Thin plumbing for tests, bench.py and the multi-GPU front end.  Nothing here
computes: staging is done by the library's host parser, synthesis by its HIP
kernels.  There is no CPU synthesis fallback - without a usable HIP device
Device() raises.
"""
import contextlib
import ctypes as C
import os

import numpy as np

from . import _build

FMT_S16LE, FMT_S16BE, FMT_U16LE, FMT_U16BE = 0, 1, 2, 3
PLAN_AUTO, PLAN_STAGEWISE = 0, 1
PLAN_FORM_ONLY, PLAN_UPLOAD_ASYNC = 0x100, 0x200          # modifiers, or-ed in (acm_hip.h)
PLAN_LEAN_ALWAYS, PLAN_NO_LEAN, PLAN_FORCE_HALO, PLAN_FORCE_CARRY = 0x400, 0x800, 0x1000, 0x2000
# test plumbing: or-ed into the flags of every Plan / batch call made through this module (fixtures that used to set ACM_K2, ACM_K1_CARRY,
# ACM_BATCH_RANGES in the environment set these instead: the shipped library reads no kernel-selection switch from the environment)
PLAN_EXTRA = 0
BATCH_EXTRA = 0
# test plumbing: True makes every helper below that works on a Device (Plan, synth, the batch, window and index calls) turn the handle's
# fill mode on first (acmhip_device_set_fill: reused arenas and recycled plan blocks start every call filled, not with the previous
# call's bytes), and synth poison its PCM buffer before it launches.  Off by default: bench.py and the measurement scripts run the library as shipped;
# tests/helpers.py turns it on for the GPU tests
FILL_MODE = False
POISON16, POISON32 = 0xA5A5, 0xFFFFFFFF         # what synth leaves in a PCM word no kernel wrote: 0xA5 bytes (16-bit formats), 0xFF bytes (float32)


def batch_ranges(n):
    """ACM_BATCH_RANGES(n) of acm_hip.h: device parsing in n block ranges (1 = in one piece, 0 = the library decides)"""
    return (int(n) & 0xFF) << 8
ERR_NO_DEVICE = -101
ERR_ARG = -103
ERR_RANGE = -105


class BlkHdr(C.Structure):
    _fields_ = [("val", C.c_uint32), ("pwr", C.c_uint32)]


class Patch(C.Structure):
    _fields_ = [("sample", C.c_uint64), ("value", C.c_int32), ("stream", C.c_uint32)]


class StreamDesc(C.Structure):
    _fields_ = [("idx_off", C.c_uint64), ("hdr_off", C.c_uint64), ("pcm_off", C.c_uint64),
                ("n_emit", C.c_uint64), ("level", C.c_uint32), ("rows", C.c_uint32),
                ("nrows", C.c_uint32), ("row_begin", C.c_uint32)]


class PlanStats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("tiles", C.c_uint64), ("fused_streams", C.c_uint32),
                ("stagewise_streams", C.c_uint32), ("launches", C.c_uint32), ("reserved", C.c_uint32),
                ("mform_tiles", C.c_uint32), ("packed_tiles", C.c_uint32)]


class PackedChunk(C.Structure):
    _fields_ = [("blob_off16", C.c_uint32), ("count", C.c_uint16), ("kind", C.c_uint8), ("row0", C.c_uint8)]


class PackedStream(C.Structure):
    _fields_ = [("chunk_off", C.c_uint64), ("ntiles", C.c_uint32), ("form", C.c_uint32)]


FORM_PACKED, FORM_BYTEPLANE = 0, 1


PACKED_CHUNK_DT = np.dtype([("blob_off16", "<u4"), ("count", "<u2"), ("kind", "u1"), ("row0", "u1")])


class StageInfo(C.Structure):
    _fields_ = [("level", C.c_uint32), ("rows", C.c_uint32), ("cols", C.c_uint32),
                ("channels", C.c_uint32), ("hdr_channels", C.c_uint32), ("rate", C.c_uint32),
                ("total_values", C.c_uint32), ("wavc", C.c_uint32), ("blocks", C.c_uint32),
                ("end_status", C.c_int32), ("npatches", C.c_uint64), ("header_bytes", C.c_uint64)]


class BatchItem(C.Structure):
    _fields_ = [("data", C.c_void_p), ("len", C.c_size_t), ("pcm", C.c_void_p), ("pcm_cap", C.c_size_t),
                ("words", C.c_uint64), ("status", C.c_int32), ("level", C.c_uint32), ("rows", C.c_uint32),
                ("channels", C.c_uint32), ("rate", C.c_uint32), ("total_values", C.c_uint32), ("reserved", C.c_uint32),
                ("dev_off", C.c_uint64)]


class BatchOpts(C.Structure):
    _fields_ = [("force_chans", C.c_int), ("fmt", C.c_uint), ("threads", C.c_int), ("plan_flags", C.c_uint),
                ("parse", C.c_uint), ("flags", C.c_uint), ("d_pcm", C.c_void_p), ("d_pcm_words", C.c_uint64),
                ("prestaged", C.c_void_p)]


class BatchTiming(C.Structure):
    _fields_ = [("stage_s", C.c_double), ("h2d_s", C.c_double), ("kernel_s", C.c_double),
                ("d2h_s", C.c_double), ("total_s", C.c_double), ("samples", C.c_uint64), ("alloc_s", C.c_double),
                ("device_parsed", C.c_uint64), ("host_parsed", C.c_uint64), ("packed_streams", C.c_uint64), ("h2d_bytes", C.c_uint64)]


class BlockMark(C.Structure):
    _fields_ = [("bit", C.c_uint64), ("val", C.c_uint32), ("pwr", C.c_uint32)]


BLOCK_MARK_DT = np.dtype([("bit", "<u8"), ("val", "<u4"), ("pwr", "<u4")])      # acm_block_mark as a numpy record: np.save / np.load keep an index


class BlockIndex(np.ndarray):
    """BLOCK_MARK_DT records that remember how their stream ends (acm_stage_info.end_status of acm_index_file): what a window that
    reaches the end of the stream reports.  A slice, a copy or an array read back from disk has forgotten it (end_status None): the
    window calls then ask the host stager, one block past the index, per call."""
    end_status = None

    def __array_finalize__(self, obj):
        self.end_status = None


def as_index(marks, end_status):
    ix = np.ascontiguousarray(marks, dtype=BLOCK_MARK_DT).view(BlockIndex)
    ix.end_status = None if end_status is None else int(end_status)
    return ix


class BatchIndex(C.Structure):
    _fields_ = [("marks", C.c_void_p), ("blocks", C.c_uint32), ("end_status", C.c_int32)]


class BatchWindow(C.Structure):
    _fields_ = [("item", C.c_uint32), ("reserved", C.c_uint32), ("first_word", C.c_uint64), ("max_words", C.c_uint64),
                ("pcm", C.c_void_p), ("pcm_cap", C.c_size_t), ("words", C.c_uint64), ("status", C.c_int32), ("reserved2", C.c_uint32),
                ("dev_off", C.c_uint64), ("slot_off", C.c_uint64), ("slot_words", C.c_uint64)]


class WindowTiming(C.Structure):
    _fields_ = [("stage_s", C.c_double), ("h2d_s", C.c_double), ("kernel_s", C.c_double), ("d2h_s", C.c_double), ("total_s", C.c_double),
                ("samples", C.c_uint64), ("alloc_s", C.c_double), ("device_parsed", C.c_uint64), ("host_parsed", C.c_uint64),
                ("h2d_bytes", C.c_uint64), ("blocks_parsed", C.c_uint64)]


class DenseOpts(C.Structure):
    _fields_ = [("frames", C.c_uint64), ("channels", C.c_uint32), ("flags", C.c_uint32), ("rate", C.c_uint32), ("reserved", C.c_uint32)]


DENSE_PLANAR = 1
DENSE_MIX = 4                   # windows of files with the other channel count are converted (mono <-> stereo), not turned away
DENSE_RESAMPLE = 16             # windows of files with another sample rate than DenseOpts.rate are resampled to it
DENSE_SPEED = 32                # BatchWindow.reserved is the window's speed num << 16 | den; ratios beyond the exact table take the wide filter


class DenseSpeedInfo(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("L", C.c_uint32), ("M", C.c_uint32), ("K", C.c_uint32), ("Wd", C.c_uint32), ("P", C.c_uint32),
                ("c", C.c_uint32), ("phases", C.c_uint32), ("step", C.c_uint64)]


SPEED_KINDS = ("none", "exact", "wide")


class OverlayRow(C.Structure):
    _fields_ = [("a", C.c_uint32), ("b", C.c_uint32), ("vol", C.c_uint32), ("snr", C.c_uint32), ("gain", C.c_uint32), ("reserved", C.c_uint32),
                ("energy_a", C.c_uint64), ("energy_b", C.c_uint64)]


OVERLAY_ROW_DT = np.dtype([("a", "<u4"), ("b", "<u4"), ("vol", "<u4"), ("snr", "<u4"), ("gain", "<u4"), ("reserved", "<u4"),
                           ("energy_a", "<u8"), ("energy_b", "<u8")])          # acm_overlay_row as a numpy record: a table of many rows at once
OVERLAY_NONE = 0xFFFFFFFF       # OverlayRow.b: nothing is laid over the row
OVERLAY_G_MAX = 32768           # the largest Q12 gain of b


class FirResponse(C.Structure):
    _fields_ = [("taps", C.c_void_p), ("ntaps", C.c_uint32), ("delay", C.c_uint32), ("shift", C.c_uint32), ("reserved", C.c_uint32)]


class FirOpts(C.Structure):
    _fields_ = [("responses", C.POINTER(FirResponse)), ("nresp", C.c_size_t), ("of_window", C.c_void_p), ("reserved", C.c_uint64)]


FIR_RESPONSE_DT = np.dtype([("taps", "<u8"), ("ntaps", "<u4"), ("delay", "<u4"), ("shift", "<u4"), ("reserved", "<u4")])   # acm_fir_response as a numpy record
FIR_NONE = 0xFFFFFFFF           # FirOpts.of_window[k]: window k is not filtered
FIR_MAX_TAPS = 32768            # of one response
FIR_MAX_L1 = 65535              # sum |h[t]| of a response at most
FIR_MAX_SHIFT = 30


class FeatBank(C.Structure):
    _fields_ = [("n_fft", C.c_uint32), ("hop", C.c_uint32), ("n_mels", C.c_uint32), ("flags", C.c_uint32), ("window", C.c_void_p), ("cs", C.c_void_p),
                ("mel_first", C.c_void_p), ("mel_count", C.c_void_p), ("mel_off", C.c_void_p), ("mel_w", C.c_void_p), ("reserved", C.c_uint64)]


class FeatLog(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("floor_q16", C.c_int32), ("mul_q24", C.c_uint32), ("offset_q16", C.c_int32), ("top_q16", C.c_uint32),
                ("reserved", C.c_uint32)]


FEAT_LOG_TOP = 1                # FeatLog.flags: clamp to the row's maximum less top_q16
FEAT_CENTER = 1                 # FeatBank.flags: frame f is centred on sample f * hop
FEAT_TIME_MAJOR = 2             # ... and the features are [row][frame][band]
FEAT_MAX_MELS = 128
FEAT_WINDOW_MAX = 32639         # the window's peak: both signed bytes of a windowed sample fit int8
FEAT_CS_ONE = 16384
FEAT_W_ONE = 32768


class BatchIndexOut(C.Structure):
    _fields_ = [("marks", C.c_void_p), ("max_blocks", C.c_size_t), ("blocks", C.c_uint32), ("end_status", C.c_int32), ("status", C.c_int32),
                ("reserved", C.c_uint32)]


class IndexOpts(C.Structure):
    _fields_ = [("force_chans", C.c_int), ("threads", C.c_int), ("parse", C.c_uint), ("reserved", C.c_uint), ("max_group_bytes", C.c_uint64)]


class IndexTiming(C.Structure):
    _fields_ = [("stage_s", C.c_double), ("h2d_s", C.c_double), ("kernel_s", C.c_double), ("d2h_s", C.c_double), ("total_s", C.c_double),
                ("blocks", C.c_uint64), ("device_indexed", C.c_uint64), ("host_indexed", C.c_uint64), ("h2d_bytes", C.c_uint64),
                ("device_bytes", C.c_uint64), ("groups", C.c_uint32), ("reserved", C.c_uint32)]


class LaunchCaps(C.Structure):
    """acmhip_launch_caps (include/acm_launch_caps.h): 0 in a field = the built-in value"""
    _fields_ = [("list_slice", C.c_uint32), ("small_grid_x", C.c_uint32), ("parse_slice", C.c_uint32), ("parse_grid_x", C.c_uint32),
                ("dense_grid", C.c_uint32)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


# the built-in values of include/acm_launch_caps.h (tests/test_launch_caps.py holds them against the header and the library)
LAUNCH_CAPS_BUILTIN = {"list_slice": 65535, "small_grid_x": 4096, "parse_slice": 65535, "parse_grid_x": 2048, "dense_grid": 1 << 20}


# every symbol include/acm_hip.h declares (checked by tests/test_abi.py)
ACMHIP_SYMBOLS = [
    "acmhip_last_error", "acmhip_device_count", "acmhip_device_open", "acmhip_device_close",
    "acmhip_device_sync", "acmhip_device_stream", "acmhip_malloc", "acmhip_free", "acmhip_host_alloc",
    "acmhip_host_free", "acmhip_upload", "acmhip_download", "acmhip_memset", "acmhip_host_synth", "acmhip_set_host_synth_limit", "acmhip_host_synth_limit", "acmhip_set_seek_index", "acmhip_plan_create", "acmhip_plan_destroy",
    "acmhip_plan_launch", "acmhip_plan_get_stats", "acmhip_plan_form_rows", "acmhip_plan_time", "acm_stage_probe", "acm_stage_file", "acm_stage_file_mform",
    "acm_batch_decode", "acm_batch_pcm_words", "acm_batch_prestage", "acm_batch_prestage_free", "acmhip_prewarm",
    "acmhip_packed_tile_rows", "acmhip_packed_group_rows", "acmhip_packed_slots", "acmhip_pack_bound", "acmhip_pack_tiles", "acmhip_unpack_tile",
    "acmhip_plan_create_packed", "acmhip_plan_bind_packed",
    "acmhip_mform_tile_rows", "acmhip_mform_group", "acmhip_mform_bytes", "acmhip_mform_pairs", "acmhip_mform_rows", "acmhip_mform_unrows", "acmhip_plan_bind_mform",
    "acmhip_plan_launch_f32", "acmhip_host_synth_f32",
    "acm_index_file", "acm_stage_window", "acm_batch_window_pcm_words", "acm_batch_decode_windows", "acm_batch_decode_windows_dense",
    "acm_dense_resampled_frames", "acm_dense_resample_taps", "acm_dense_speed_frames", "acm_dense_speed_taps",
    "acm_batch_decode_windows_overlay", "acm_dense_overlay_gain", "acm_batch_decode_windows_overlay_fir", "acm_dense_fir_check",
    "acm_batch_decode_windows_features", "acm_feat_bank_check", "acm_feat_frames", "acm_feat_design",
    "acm_batch_decode_windows_logmel", "acm_feat_log_check",
    "acm_batch_index_blocks", "acm_batch_index_files", "acm_batch_decode_indexed", "acm_batch_prestaged_index",
    "acmhip_device_set_fill", "acmhip_device_arena_info", "acmhip_device_set_launch_caps",
]
# the 19 entry points of include/libacm.h (reference src/libacm.h:120-170)
LIBACM_SYMBOLS = [
    "acm_open_decoder", "acm_read", "acm_close", "acm_open_file", "acm_info", "acm_seekable", "acm_bitrate",
    "acm_rate", "acm_channels", "acm_raw_total", "acm_raw_tell", "acm_pcm_total", "acm_pcm_tell",
    "acm_time_total", "acm_time_tell", "acm_read_loop", "acm_seek_pcm", "acm_seek_time", "acm_strerror",
]

_lib = None


def lib_path():
    return os.path.join(_build.LIB, "libacm_hip.so")


def lib():
    """Load libacm_hip.so (building it if the tree is newer)."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: the PyTorch wheel bundles its own libamdhip64.so.7; if the system copy
    # gets loaded first (through libacm_hip.so's DT_NEEDED) and torch later brings its own, the second one
    # finds no GPUs.  Importing torch first makes the loader resolve our DT_NEEDED to the copy already mapped.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    path = os.environ.get("ACM_HIP_LIB") or _build.build_hip()      # ACM_HIP_LIB: A/B runs of experimental builds
    L = C.CDLL(path)
    vp, sz = C.c_void_p, C.c_size_t
    L.acmhip_last_error.restype = C.c_char_p
    L.acmhip_device_open.argtypes = [C.c_int, vp, C.POINTER(vp)]
    L.acmhip_device_close.argtypes = [vp]
    L.acmhip_device_close.restype = None
    L.acmhip_device_sync.argtypes = [vp]
    L.acmhip_device_stream.argtypes = [vp]
    L.acmhip_device_stream.restype = vp
    L.acmhip_device_set_fill.argtypes = [vp, C.c_int]
    L.acmhip_device_arena_info.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    if hasattr(L, "acmhip_device_set_launch_caps"):                # (an older library named by ACM_HIP_LIB for an A/B run has none)
        L.acmhip_device_set_launch_caps.argtypes = [vp, C.POINTER(LaunchCaps), C.POINTER(LaunchCaps)]
        L.acmk_launch_caps_set.argtypes = [C.POINTER(LaunchCaps)] * 3
    L.acmhip_malloc.argtypes = [vp, sz, C.POINTER(vp)]
    L.acmhip_free.argtypes = [vp, vp]
    L.acmhip_host_alloc.argtypes = [sz, C.POINTER(vp)]
    L.acmhip_host_free.argtypes = [vp]
    L.acmhip_upload.argtypes = [vp, vp, vp, sz]
    L.acmhip_download.argtypes = [vp, vp, vp, sz]
    L.acmhip_memset.argtypes = [vp, vp, C.c_int, sz]
    L.acmhip_host_synth.argtypes = [C.POINTER(StreamDesc), vp, vp, vp, sz, C.c_uint, vp]
    L.acmhip_host_synth_f32.argtypes = [C.POINTER(StreamDesc), vp, vp, vp, sz, vp]
    L.acmhip_set_host_synth_limit.argtypes = [C.c_uint64]
    L.acmhip_set_host_synth_limit.restype = None
    L.acmhip_host_synth_limit.restype = C.c_uint64
    L.acmhip_set_seek_index.argtypes = [C.c_int]
    L.acmhip_set_seek_index.restype = None
    L.acmhip_plan_create.argtypes = [vp, C.POINTER(StreamDesc), sz, C.POINTER(Patch), sz, C.c_uint, C.POINTER(vp)]
    L.acmhip_plan_destroy.argtypes = [vp]
    L.acmhip_plan_destroy.restype = None
    L.acmhip_plan_launch.argtypes = [vp, vp, vp, vp, C.c_uint]
    L.acmhip_plan_launch_f32.argtypes = [vp, vp, vp, vp]
    L.acmhip_plan_get_stats.argtypes = [vp, C.POINTER(PlanStats)]
    L.acmhip_plan_form_rows.argtypes = [vp, C.c_size_t, C.POINTER(C.c_uint64)]
    L.acmhip_plan_time.argtypes = [vp, vp, vp, vp, C.c_uint, C.c_int, C.POINTER(C.c_float)]
    L.acm_stage_probe.argtypes = [vp, sz, C.c_int, C.POINTER(StageInfo)]
    L.acm_stage_file.argtypes = [vp, sz, C.c_int, vp, vp, sz, vp, sz, C.POINTER(StageInfo)]
    L.acm_stage_file_mform.argtypes = [vp, sz, C.c_int, vp, vp, sz, C.POINTER(StageInfo), vp, C.c_uint64, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.acm_batch_decode.argtypes = [vp, C.POINTER(BatchItem), sz, C.POINTER(BatchOpts), C.POINTER(BatchTiming)]
    L.acm_batch_pcm_words.argtypes = [C.POINTER(BatchItem), sz, C.c_int]
    L.acm_batch_pcm_words.restype = C.c_uint64
    L.acm_batch_prestage.argtypes = [C.POINTER(BatchItem), sz, C.POINTER(BatchOpts), C.POINTER(vp), C.POINTER(C.c_double)]
    L.acm_batch_prestage_free.argtypes = [vp]
    L.acm_batch_prestage_free.restype = None
    L.acmhip_packed_tile_rows.argtypes = [C.c_uint32]
    L.acmhip_packed_group_rows.argtypes = [C.c_uint32]
    L.acmhip_packed_slots.argtypes = [C.c_uint32]
    L.acmhip_pack_bound.argtypes = [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]
    L.acmhip_pack_tiles.argtypes = [C.c_uint32, vp, C.c_uint64, vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    L.acmhip_unpack_tile.argtypes = [C.c_uint32, vp, vp, vp]
    L.acmhip_plan_create_packed.argtypes = [vp, C.POINTER(StreamDesc), sz, C.POINTER(PackedStream), C.POINTER(Patch), sz, C.c_uint, C.POINTER(vp)]
    L.acmhip_plan_bind_packed.argtypes = [vp, vp, vp]
    L.acmhip_mform_tile_rows.argtypes = [C.c_uint32]
    L.acmhip_mform_group.argtypes = [C.c_uint32]
    L.acmhip_mform_bytes.argtypes = [C.c_uint32, C.c_uint64]
    L.acmhip_mform_bytes.restype = C.c_uint64
    L.acmhip_mform_pairs.argtypes = [C.c_uint64]
    L.acmhip_mform_pairs.restype = C.c_uint64
    L.acmhip_mform_rows.argtypes = [C.c_uint32, vp, C.c_uint64, vp, C.c_uint64, vp, C.POINTER(C.c_uint64)]
    L.acmhip_mform_unrows.argtypes = [C.c_uint32, vp, vp, C.c_uint64, vp]
    L.acmhip_plan_bind_mform.argtypes = [vp, vp, vp]
    L.acm_index_file.argtypes = [vp, sz, C.c_int, vp, sz, C.POINTER(StageInfo)]
    L.acm_stage_window.argtypes = [vp, sz, C.c_int, vp, sz, C.c_uint32, C.c_uint32, vp, vp, vp, sz, C.POINTER(StageInfo)]
    L.acm_batch_window_pcm_words.argtypes = [C.POINTER(BatchItem), sz, C.POINTER(BatchWindow), sz, C.c_int]
    L.acm_batch_window_pcm_words.restype = C.c_uint64
    L.acm_batch_decode_windows.argtypes = [vp, C.POINTER(BatchItem), sz, C.POINTER(BatchIndex), C.POINTER(BatchWindow), sz,
                                           C.POINTER(BatchOpts), C.POINTER(WindowTiming)]
    L.acm_batch_decode_windows_dense.argtypes = [vp, C.POINTER(BatchItem), sz, C.POINTER(BatchIndex), C.POINTER(BatchWindow), sz,
                                                 C.POINTER(BatchOpts), C.POINTER(DenseOpts), C.POINTER(WindowTiming)]
    if hasattr(L, "acm_dense_resampled_frames"):                   # (an older library named by ACM_HIP_LIB for an A/B run has none)
        L.acm_dense_resampled_frames.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
        L.acm_dense_resampled_frames.restype = C.c_uint64
        L.acm_dense_resample_taps.argtypes = [C.c_uint32, C.c_uint32] + [C.POINTER(C.c_uint32)] * 4 + [vp, sz]
    if hasattr(L, "acm_dense_speed_frames"):
        L.acm_dense_speed_frames.argtypes = [C.c_uint64] + [C.c_uint32] * 4
        L.acm_dense_speed_frames.restype = C.c_uint64
        L.acm_dense_speed_taps.argtypes = [C.c_uint32] * 4 + [C.POINTER(DenseSpeedInfo), vp, sz]
    if hasattr(L, "acm_batch_decode_windows_overlay"):
        L.acm_batch_decode_windows_overlay.argtypes = [vp, C.POINTER(BatchItem), sz, C.POINTER(BatchIndex), C.POINTER(BatchWindow), sz,
                                                       C.POINTER(BatchOpts), C.POINTER(DenseOpts), C.POINTER(OverlayRow), sz, C.POINTER(WindowTiming)]
        L.acm_dense_overlay_gain.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
        L.acm_dense_overlay_gain.restype = C.c_uint32
    if hasattr(L, "acm_batch_decode_windows_overlay_fir"):
        L.acm_batch_decode_windows_overlay_fir.argtypes = [vp, C.POINTER(BatchItem), sz, C.POINTER(BatchIndex), C.POINTER(BatchWindow), sz,
                                                           C.POINTER(BatchOpts), C.POINTER(DenseOpts), C.POINTER(FirOpts), C.POINTER(OverlayRow), sz,
                                                           C.POINTER(WindowTiming)]
        L.acm_dense_fir_check.argtypes = [C.POINTER(FirResponse)]
    if hasattr(L, "acm_batch_decode_windows_features"):
        L.acm_batch_decode_windows_features.argtypes = [vp, C.POINTER(BatchItem), sz, C.POINTER(BatchIndex), C.POINTER(BatchWindow), sz,
                                                        C.POINTER(BatchOpts), C.POINTER(DenseOpts), C.POINTER(FirOpts), C.POINTER(FeatBank),
                                                        C.POINTER(OverlayRow), sz, C.POINTER(WindowTiming)]
        L.acm_feat_bank_check.argtypes = [C.POINTER(FeatBank)]
        L.acm_feat_frames.argtypes = [C.c_uint64, C.POINTER(FeatBank)]
        L.acm_feat_frames.restype = C.c_uint64
        L.acm_feat_design.argtypes = [C.c_uint32] * 5 + [C.c_double, C.c_double, C.c_uint32] + [vp] * 6 + [sz, C.POINTER(sz)]
    if hasattr(L, "acm_batch_decode_windows_logmel"):
        L.acm_batch_decode_windows_logmel.argtypes = [vp, C.POINTER(BatchItem), sz, C.POINTER(BatchIndex), C.POINTER(BatchWindow), sz,
                                                      C.POINTER(BatchOpts), C.POINTER(DenseOpts), C.POINTER(FirOpts), C.POINTER(FeatBank),
                                                      C.POINTER(FeatLog), C.POINTER(OverlayRow), sz, C.POINTER(WindowTiming)]
        L.acm_feat_log_check.argtypes = [C.POINTER(FeatBank), C.POINTER(FeatLog)]
    L.acm_batch_index_blocks.argtypes = [C.POINTER(BatchItem), sz, C.c_int, vp]
    L.acm_batch_index_blocks.restype = C.c_uint64
    L.acm_batch_index_files.argtypes = [vp, C.POINTER(BatchItem), sz, C.POINTER(BatchIndexOut), C.POINTER(IndexOpts), C.POINTER(IndexTiming)]
    L.acm_batch_decode_indexed.argtypes = [vp, C.POINTER(BatchItem), sz, C.POINTER(BatchOpts), C.POINTER(BatchIndexOut), C.POINTER(BatchTiming)]
    L.acm_batch_prestaged_index.argtypes = [vp, sz, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]
    _lib = L
    return L


class AcmHipError(RuntimeError):
    pass


def _check(rc, what):
    if rc != 0:
        raise AcmHipError("%s failed (%d): %s" % (what, rc, lib().acmhip_last_error().decode(errors="replace")))


def device_count():
    return lib().acmhip_device_count()


# --------------------------------------------------------------------------- host staging
class Staged:
    """One file in staged form: idx (int16, PCM order), hdr (uint32[blocks,2] = val,pwr), patches, info."""

    def __init__(self, idx, hdr, patches, info):
        self.idx, self.hdr, self.patches, self.info = idx, hdr, patches, info

    @property
    def block_len(self):
        return self.info.rows * self.info.cols

    @property
    def words(self):
        """words an acm_read_loop() caller would get (whole blocks, total_values cut, channel rounding)"""
        pos, bl, tot, ch = 0, self.block_len, self.info.total_values, self.info.channels
        for _ in range(self.info.blocks):
            if pos >= tot:
                break
            take = min(bl, tot - pos)
            if ch > 1:
                take -= take % ch
            pos += take
            if take != bl:
                break
        return pos


def _as_u8(data):
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8)
    return np.frombuffer(bytes(data), dtype=np.uint8)


def probe(data, force_chans=0):
    a = _as_u8(data)
    info = StageInfo()
    rc = lib().acm_stage_probe(a.ctypes.data, a.size, force_chans, C.byref(info))
    return rc, info


def header_channels(files, which=None, force_chans=0):
    """{file number: channels the header of files[number] says} for the numbers in `which` (default: all) whose file is ACM - the
    probe of probe(); no file image is copied"""
    return _header_field(files, which, force_chans, "channels")


def header_rates(files, which=None, force_chans=0):
    """header_channels' sibling: {file number: the sample rate the header of files[number] says}"""
    return _header_field(files, which, force_chans, "rate")


def _header_field(files, which, force_chans, field):
    probe_fn, info, out = lib().acm_stage_probe, StageInfo(), {}
    ref = C.byref(info)
    for f in range(len(files)) if which is None else which:
        data = files[f]
        if isinstance(data, bytes):
            rc = probe_fn(data, len(data), force_chans, ref)
        else:
            a = _as_u8(data) if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)
            rc = probe_fn(a.ctypes.data, a.size, force_chans, ref)
        if rc == 0:
            out[f] = getattr(info, field)
    return out


def dense_resampled_frames(source_frames, rate_in, rate_out):
    """acm_dense_resampled_frames: the frames of a row of ACM_DENSE_RESAMPLE made of source_frames frames, None for a ratio the dense
    writer does not take"""
    n = lib().acm_dense_resampled_frames(source_frames, rate_in, rate_out)
    return None if n == 2 ** 64 - 1 else int(n)


def dense_resample_taps(rate_in, rate_out):
    """acm_dense_resample_taps -> (L, M, K, Wd, the Q14 table as an int16 array [L, K]); ValueError for a ratio that is not supported"""
    n = [C.c_uint32() for _ in range(4)]
    refs = [C.byref(v) for v in n]
    if lib().acm_dense_resample_taps(rate_in, rate_out, *refs, None, 0) != 0:
        raise ValueError("acm_dense_resample_taps: %d -> %d is not a supported ratio" % (rate_in, rate_out))
    L, M, K, Wd = (int(v.value) for v in n)
    taps = np.zeros((L, K), dtype=np.int16)
    _check(lib().acm_dense_resample_taps(rate_in, rate_out, *refs, taps.ctypes.data, taps.size), "acm_dense_resample_taps")
    return L, M, K, Wd, taps


def dense_speed_frames(source_frames, rate_in, rate_out, speed=(1, 1)):
    """acm_dense_speed_frames: the frames of a row of ACM_DENSE_SPEED made of source_frames frames of a file at rate_in played at
    speed = (num, den), None where the window would be turned away"""
    n = lib().acm_dense_speed_frames(source_frames, rate_in, rate_out, speed[0], speed[1])
    return None if n == 2 ** 64 - 1 else int(n)


def dense_speed_taps(rate_in, rate_out, speed=(1, 1)):
    """acm_dense_speed_taps -> (DenseSpeedInfo, the Q14 table the kernel reads as an int16 array [phases, K]); info.kind indexes
    SPEED_KINDS.  ValueError where the window would be turned away"""
    info = DenseSpeedInfo()
    if lib().acm_dense_speed_taps(rate_in, rate_out, speed[0], speed[1], C.byref(info), None, 0) != 0:
        raise ValueError("acm_dense_speed_taps: %d -> %d at %d/%d is turned away" % (rate_in, rate_out, speed[0], speed[1]))
    taps = np.zeros((info.phases, info.K), dtype=np.int16)
    _check(lib().acm_dense_speed_taps(rate_in, rate_out, speed[0], speed[1], None, taps.ctypes.data, taps.size), "acm_dense_speed_taps")
    return info, taps


def stage_file(data, force_chans=0, idx_out=None, hdr_out=None):
    """Host bit parsing of a whole file image -> Staged (raises on a non-ACM file)."""
    a = _as_u8(data)
    rc, info = probe(a, force_chans)
    if rc != 0:
        raise ValueError("not an ACM stream (%d)" % rc)
    bl = info.rows * info.cols
    need = (info.total_values + bl - 1) // bl
    idx = idx_out if idx_out is not None else np.zeros(need * bl, dtype=np.int16)
    hdr = hdr_out if hdr_out is not None else np.zeros((need, 2), dtype=np.uint32)
    assert idx.size >= need * bl and hdr.shape[0] >= need
    info2 = StageInfo()
    rc = lib().acm_stage_file(a.ctypes.data, a.size, force_chans, idx.ctypes.data, hdr.ctypes.data, need,
                              None, 0, C.byref(info2))
    if rc != 0:
        raise ValueError("acm_stage_file failed (%d)" % rc)
    patches = None
    if info2.npatches:
        patches = (Patch * info2.npatches)()
        rc = lib().acm_stage_file(a.ctypes.data, a.size, force_chans, idx.ctypes.data, hdr.ctypes.data, need,
                                  patches, info2.npatches, C.byref(info2))
    return Staged(idx[:info2.blocks * bl], hdr[:info2.blocks], patches, info2)


def stage_file_mform(data, force_chans=0, mf_base=0):
    """acm_stage_file_mform: the byte-plane form written by the parsing pass itself.  Returns (info, idx, hdr, blob, pairs, mf_rows, mf_bytes);
    idx is filled with -12345 beforehand, so the rows the call leaves alone show."""
    a = _as_u8(data)
    rc, info = probe(a, force_chans)
    if rc != 0:
        raise ValueError("not an ACM stream (%d)" % rc)
    bl = info.rows * info.cols
    need = (info.total_values + bl - 1) // bl
    idx = np.full(need * bl, -12345, dtype=np.int16)
    hdr = np.zeros((need, 2), dtype=np.uint32)
    nrows = (need * info.rows) & ~1
    blob = np.zeros(int(lib().acmhip_mform_bytes(info.level, nrows)) + 256, dtype=np.uint8)
    pairs = np.zeros(int(lib().acmhip_mform_pairs(nrows)) + 32, dtype=np.uint32)
    info2 = StageInfo()
    rows, nbytes = C.c_uint64(), C.c_uint64()
    rc = lib().acm_stage_file_mform(a.ctypes.data, a.size, force_chans, idx.ctypes.data, hdr.ctypes.data, need, C.byref(info2),
                                    blob.ctypes.data, mf_base, pairs.ctypes.data, C.byref(rows), C.byref(nbytes))
    if rc != 0:
        raise ValueError("acm_stage_file_mform failed (%d)" % rc)
    return info2, idx, hdr, blob, pairs, rows.value, nbytes.value


# --------------------------------------------------------------------------- block index
def index_file(data, force_chans=0):
    """acm_index_file: the block index of a file image -> (marks, info).  marks: BLOCK_MARK_DT records, info.blocks + 1 of them (the
    last one: the bit behind the last whole block); info: what acm_stage_file reports for the same bytes.  Raises on a non-ACM file."""
    a = _as_u8(data)
    rc, info = probe(a, force_chans)
    if rc != 0:
        raise ValueError("not an ACM stream (%d)" % rc)
    bl = info.rows * info.cols
    need = (info.total_values + bl - 1) // bl
    # (the header may promise far more blocks than the bytes can hold: a block costs at least its header and a code per column)
    need = min(need, (max(0, a.size - info.header_bytes) * 8 + 8) // (20 + 5 * info.cols) + 1)
    marks = np.zeros(need + 1, dtype=BLOCK_MARK_DT)
    info2 = StageInfo()
    rc = lib().acm_index_file(a.ctypes.data, a.size, force_chans, marks.ctypes.data, need, C.byref(info2))
    if rc != 0:
        raise ValueError("acm_index_file failed (%d)" % rc)
    return as_index(marks[:info2.blocks + 1].copy(), info2.end_status), info2


def stage_window(data, marks, block_first, block_count, force_chans=0, nblocks_indexed=None):
    """acm_stage_window: blocks [block_first, block_first + block_count) of a file entered through its index ->
    (rc, Staged or None).  Staged.info.blocks = blocks staged, .info.end_status = what stopped it; patch samples count from the first
    staged sample."""
    a = _as_u8(data)
    rc, info = probe(a, force_chans)
    if rc != 0:
        return rc, None
    marks = np.ascontiguousarray(marks, dtype=BLOCK_MARK_DT)
    nidx = marks.size - 1 if nblocks_indexed is None else nblocks_indexed
    bl = info.rows * info.cols
    idx = np.zeros(max(block_count, 1) * bl, dtype=np.int16)
    hdr = np.zeros((max(block_count, 1), 2), dtype=np.uint32)
    info2 = StageInfo()
    rc = lib().acm_stage_window(a.ctypes.data, a.size, force_chans, marks.ctypes.data, nidx, block_first, block_count,
                                idx.ctypes.data, hdr.ctypes.data, None, 0, C.byref(info2))
    if rc != 0:
        return rc, None
    patches = None
    if info2.npatches:
        patches = (Patch * info2.npatches)()
        rc = lib().acm_stage_window(a.ctypes.data, a.size, force_chans, marks.ctypes.data, nidx, block_first, block_count,
                                    idx.ctypes.data, hdr.ctypes.data, patches, info2.npatches, C.byref(info2))
    return rc, Staged(idx[:info2.blocks * bl], hdr[:info2.blocks], patches, info2)


# --------------------------------------------------------------------------- host staging, packed half
def packed_tile_rows(level):
    return lib().acmhip_packed_tile_rows(level)


class PackedArena:
    """Host tables of the packed staged form of several streams: .chunks (acmhip_packed_slots(level) entries per tile), .blob,
    and .streams (PackedStream beside each stream descriptor)."""

    def __init__(self, chunks, blob, streams):
        self.chunks, self.blob, self.streams = chunks, blob, streams

    def upload(self, dev):
        ptrs = []
        for a in (self.chunks, self.blob):
            p = dev.malloc(max(a.nbytes, 16))
            flat = a.view(np.uint8).reshape(-1)
            for o in range(0, flat.size, 1 << 28):
                dev.upload(p + o, flat[o:o + (1 << 28)])
            ptrs.append(p)
        return tuple(ptrs)

    @property
    def nbytes(self):
        return self.chunks.nbytes + self.blob.nbytes


class MformArena:
    """The byte-plane staged form (acmhip_mform_rows) of several streams: .data (uint8 arena), .pairs (uint32 pair table: offset in
    64-byte units << 2 | width class) and .streams (PackedStream with form = FORM_BYTEPLANE beside each stream descriptor)."""

    def __init__(self, data, pairs, streams):
        self.data, self.pairs, self.streams = data, pairs, streams

    def upload(self, dev):
        ptrs = []
        for a in (self.data, self.pairs):
            p = dev.malloc(max(a.nbytes, 16))
            flat = a.view(np.uint8).reshape(-1)
            for o in range(0, flat.size, 1 << 28):
                dev.upload(p + o, flat[o:o + (1 << 28)])
            ptrs.append(p)
        return tuple(ptrs)

    @property
    def nbytes(self):
        return self.data.nbytes + self.pairs.nbytes

    def class_counts(self):
        """pair-table entries per class code: 1 = 12 bits at levels 8-12 (4 bits in level 7's form), 2 = 8 bits, 3 = 16 bits as two signed
        bytes; 0 = 16 bits over the whole int16 range at levels 8-12 - and the table's 32 entries of read slack, which are zeros"""
        return np.bincount(self.pairs & 3, minlength=4)


def mform_streams(idx, descs, threads=1, L=None):
    """The byte-plane form of every stream of a staged arena that can have one (whole tiles from row 0 of the levels
    acmhip_mform_tile_rows() covers).  L: another build of the library to stage with (profiles/ab_kernels.py --own-form)."""
    from concurrent.futures import ThreadPoolExecutor
    L = L or lib()
    n = len(descs)
    ntiles, rows, cap, p_at = [0] * n, [0] * n, [0] * n, [0] * n
    np_tot = 0
    for i, d in enumerate(descs):
        tr = L.acmhip_mform_tile_rows(d.level)
        if tr > 0 and d.row_begin == 0:
            ntiles[i] = min(d.nrows, d.n_emit >> d.level) // tr
            if (ntiles[i] * tr) & 1:            # the form is written pair by pair (chunks of one row: an even number of them)
                ntiles[i] -= 1
            rows[i] = ntiles[i] * tr
        p_at[i] = np_tot
        if ntiles[i]:
            cap[i] = (L.acmhip_mform_bytes(d.level, rows[i]) + 255) // 256 * 256
            np_tot += L.acmhip_mform_pairs(rows[i])
    pairs = np.zeros(np_tot + 32, dtype=np.uint32)             # (the kernel's scalar loads fetch whole groups of entries)
    parts = [None] * n

    def one(i):
        if ntiles[i]:
            d = descs[i]
            buf = np.empty(cap[i], dtype=np.uint8)
            used = C.c_uint64()
            rc = L.acmhip_mform_rows(d.level, idx[d.idx_off:].ctypes.data, rows[i], buf.ctypes.data, 0, pairs[p_at[i]:].ctypes.data,
                                     C.byref(used))
            if rc == ERR_RANGE:                 # (libraries of rounds 5 / 6, A/B runs: an index the form could not hold - the stream stays int16)
                ntiles[i] = 0
                return
            _check(rc, "acmhip_mform_rows")
            parts[i] = buf[:(used.value + 63) // 64 * 64]
    with ThreadPoolExecutor(max_workers=max(1, threads)) as ex:
        list(ex.map(one, range(n)))
    total = sum(p.size for p in parts if p is not None)
    if (total >> 6) >= 1 << 30:
        raise AcmHipError("byte-plane arena beyond 64 GB")
    at = 0
    for i in range(n):
        if parts[i] is not None:
            k = int(L.acmhip_mform_pairs(rows[i]))
            pairs[p_at[i]:p_at[i] + k] += np.uint32((at // 64) << 2)        # offsets were written relative to the stream's own block
            at += parts[i].size
    data = np.empty(max(at, 16) + 64, dtype=np.uint8)
    at = 0
    for i in range(n):
        if parts[i] is not None:
            data[at:at + parts[i].size] = parts[i]
            at += parts[i].size
    data[at:] = 0
    return MformArena(data, pairs, [PackedStream(p_at[i], ntiles[i], FORM_BYTEPLANE) for i in range(n)])


def mform_unrows(level, blob, pairs, nrows):
    out = np.zeros(nrows << level, dtype=np.int16)
    _check(lib().acmhip_mform_unrows(level, blob.ctypes.data, pairs.ctypes.data, nrows, out.ctypes.data), "acmhip_mform_unrows")
    return out


def pack_streams(idx, descs, threads=1):
    """The packed staged form of every stream of a staged arena that can have one (whole tiles from row 0 of the levels
    acmhip_packed_tile_rows() covers): returns a PackedArena whose .streams is a list of PackedStream beside descs."""
    from concurrent.futures import ThreadPoolExecutor
    L = lib()
    n = len(descs)
    ntiles, chunk_off, blob_cap, slots = [0] * n, [0] * n, [0] * n, [0] * n
    c_at = 0
    for i, d in enumerate(descs):
        tr = L.acmhip_packed_tile_rows(d.level)
        if tr > 0 and d.row_begin == 0:
            ntiles[i] = min(d.nrows, d.n_emit >> d.level) // tr
            slots[i] = L.acmhip_packed_slots(d.level)
        chunk_off[i] = c_at
        c_at += ntiles[i] * slots[i]
        if ntiles[i]:
            mb = C.c_uint64()
            _check(L.acmhip_pack_bound(d.level, ntiles[i], C.byref(mb)), "acmhip_pack_bound")
            blob_cap[i] = (mb.value + 15) // 16 * 16
    chunks = np.zeros(max(c_at, 1), dtype=PACKED_CHUNK_DT)
    parts = [None] * n

    def one(i):
        if not ntiles[i]:
            return
        d = descs[i]
        bl = np.zeros(blob_cap[i], dtype=np.uint8)
        nb = C.c_uint64()
        _check(L.acmhip_pack_tiles(d.level, idx[d.idx_off:].ctypes.data, ntiles[i], chunks[chunk_off[i]:].ctypes.data,
                                   bl.ctypes.data, 0, C.byref(nb)), "acmhip_pack_tiles")
        parts[i] = bl[:nb.value].copy()
    with ThreadPoolExecutor(max_workers=max(1, threads)) as ex:
        list(ex.map(one, range(n)))
    b_at = 0
    lay = []
    for i in range(n):
        lay.append(b_at)
        if parts[i] is not None:
            b_at += (parts[i].size + 15) // 16 * 16
    blob = np.zeros(max(b_at, 16), dtype=np.uint8)
    for i in range(n):
        if parts[i] is None:
            continue
        b0 = lay[i]
        c = chunks[chunk_off[i]:chunk_off[i] + ntiles[i] * slots[i]]
        c["blob_off16"][c["kind"] != 0] += b0 // 16
        blob[b0:b0 + parts[i].size] = parts[i]
        parts[i] = None
    streams = [PackedStream(chunk_off[i], ntiles[i], 0) for i in range(n)]
    return PackedArena(chunks, blob, streams)


def unpack_tile(level, chunks, blob, entry):
    """inverse of the packer for the tile whose descriptors start at chunk-table entry `entry` (tests): int16 [tile_rows, cols]"""
    tr = lib().acmhip_packed_tile_rows(level)
    out = np.zeros((tr, 1 << level), dtype=np.int16)
    _check(lib().acmhip_unpack_tile(level, chunks[entry:].ctypes.data, blob.ctypes.data, out.ctypes.data), "acmhip_unpack_tile")
    return out


# --------------------------------------------------------------------------- device
class Device:
    def __init__(self, ordinal=0, hip_stream=None):
        self.h = C.c_void_p()
        self.fill = False               # the handle's fill mode as set_fill left it
        rc = lib().acmhip_device_open(ordinal, hip_stream, C.byref(self.h))
        if rc != 0:
            self.h = None
            raise AcmHipError("acmhip_device_open(%d) failed (%d): %s"
                              % (ordinal, rc, lib().acmhip_last_error().decode(errors="replace")))

    def close(self):
        if self.h:
            lib().acmhip_device_close(self.h)
            self.h = None

    def set_fill(self, on):
        """acmhip_device_set_fill: the handle's fill mode on / off -> its previous state"""
        was = lib().acmhip_device_set_fill(self.h, 1 if on else 0)
        if was < 0:
            _check(was, "acmhip_device_set_fill")
        self.fill = bool(on)
        return bool(was)

    def set_launch_caps(self, caps=None):
        """acmhip_device_set_launch_caps: caps = a LaunchCaps, a dict of its fields, or None for the built-in values -> the LaunchCaps in
        force before"""
        if isinstance(caps, dict):
            caps = LaunchCaps(**caps)
        was = LaunchCaps()
        _check(lib().acmhip_device_set_launch_caps(self.h, C.byref(caps) if caps is not None else None, C.byref(was)),
               "acmhip_device_set_launch_caps")
        return was

    @contextlib.contextmanager
    def launch_caps(self, **fields):
        """tests only: the handle's launch caps lowered to `fields` (list_slice=3, dense_grid=1, ...; the others built-in) inside the
        with block, the previous caps back behind it"""
        was = self.set_launch_caps(LaunchCaps(**fields))
        try:
            yield
        finally:
            self.set_launch_caps(was)

    def arena_info(self):
        """acmhip_device_arena_info over every staging arena of the handle -> {name: (slot, ptr or None, bytes the last call asked of it,
        is_host, fill byte)}"""
        out, slot = {}, 0
        name, ptr, nbytes, host, fill = C.c_char_p(), C.c_void_p(), C.c_size_t(), C.c_int(), C.c_int()
        while lib().acmhip_device_arena_info(self.h, slot, C.byref(name), C.byref(ptr), C.byref(nbytes), C.byref(host), C.byref(fill)) == 0:
            out[name.value.decode()] = (slot, ptr.value, int(nbytes.value), bool(host.value), int(fill.value))
            slot += 1
        return out

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def sync(self):
        _check(lib().acmhip_device_sync(self.h), "acmhip_device_sync")

    def malloc(self, nbytes):
        p = C.c_void_p()
        _check(lib().acmhip_malloc(self.h, nbytes, C.byref(p)), "acmhip_malloc")
        return p.value

    def free(self, ptr):
        if ptr:
            _check(lib().acmhip_free(self.h, ptr), "acmhip_free")

    def upload(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        _check(lib().acmhip_upload(self.h, dptr, arr.ctypes.data, arr.nbytes), "acmhip_upload")
        self.sync()          # pageable numpy memory: finish before the array can go away

    def download(self, arr, dptr):
        _check(lib().acmhip_download(self.h, arr.ctypes.data, dptr, arr.nbytes), "acmhip_download")
        self.sync()

    def memset(self, dptr, byte, nbytes):
        """fill device memory (queued on the device stream); the parity tests poison a whole PCM arena with it before a launch"""
        _check(lib().acmhip_memset(self.h, dptr, byte, nbytes), "acmhip_memset")


def _fill(dev):
    """FILL_MODE: the handle's fill mode goes on with the first helper that is given the handle"""
    if FILL_MODE and dev is not None and getattr(dev, "h", None) and not getattr(dev, "fill", False):
        dev.set_fill(True)


class Plan:
    def __init__(self, dev, descs, patches=None, flags=PLAN_AUTO, packed=None):
        """packed: optional list of PackedStream, one per desc (ntiles 0 = that stream has no packed form)"""
        self.dev = dev
        _fill(dev)
        flags |= PLAN_EXTRA
        n = len(descs)
        arr = (StreamDesc * max(n, 1))(*descs)
        np_ = len(patches) if patches is not None else 0
        self.h = C.c_void_p()
        if packed is not None:
            assert len(packed) == n
            pk = (PackedStream * max(n, 1))(*packed)
            _check(lib().acmhip_plan_create_packed(dev.h, arr, n, pk, patches if np_ else None, np_, flags, C.byref(self.h)),
                   "acmhip_plan_create_packed")
        else:
            _check(lib().acmhip_plan_create(dev.h, arr, n, patches if np_ else None, np_, flags, C.byref(self.h)),
                   "acmhip_plan_create")

    def bind_packed(self, d_chunks, d_blob):
        """device tables of the packed staged form for every later launch (both None: back to the int16 arena)"""
        _check(lib().acmhip_plan_bind_packed(self.h, d_chunks, d_blob), "acmhip_plan_bind_packed")

    def bind_mform(self, d_mform, d_pairs):
        """device arena and pair table of the byte-plane staged form for every later launch (both None: back to the int16 arena)"""
        _check(lib().acmhip_plan_bind_mform(self.h, d_mform, d_pairs), "acmhip_plan_bind_mform")

    def launch(self, d_idx, d_hdr, d_pcm, fmt=FMT_S16LE):
        _check(lib().acmhip_plan_launch(self.h, d_idx, d_hdr, d_pcm, fmt), "acmhip_plan_launch")

    def launch_f32(self, d_idx, d_hdr, d_pcm):
        """float32 samples (the s16le sample times 2^-15, exactly) into d_pcm; the descriptors' pcm_off / n_emit count floats"""
        _check(lib().acmhip_plan_launch_f32(self.h, d_idx, d_hdr, d_pcm), "acmhip_plan_launch_f32")

    def time(self, d_idx, d_hdr, d_pcm, fmt=FMT_S16LE, reps=1):
        ms = C.c_float()
        _check(lib().acmhip_plan_time(self.h, d_idx, d_hdr, d_pcm, fmt, reps, C.byref(ms)), "acmhip_plan_time")
        return ms.value

    def stats(self):
        st = PlanStats()
        _check(lib().acmhip_plan_get_stats(self.h, C.byref(st)), "acmhip_plan_get_stats")
        return st

    def form_rows(self, stream):
        """rows of stream `stream` this plan reads from the stream's second staged form (0: none of them)"""
        rows = C.c_uint64()
        _check(lib().acmhip_plan_form_rows(self.h, stream, C.byref(rows)), "acmhip_plan_form_rows")
        return rows.value

    def destroy(self):
        if self.h:
            # a plan that outlived its device handle (a test that failed before its destroy(), collected at interpreter exit) is the
            # handle's memory gone with it: nothing left to hand back, and the handle must not be touched
            if getattr(self.dev, "h", None):
                lib().acmhip_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def _round_up(v, a):
    return (v + a - 1) // a * a


class Arena:
    """Several staged streams laid out in three host arrays + their descriptors (whole-stream decode)."""

    def __init__(self, staged_list, windows=None):
        """windows: optional per-stream (row_begin, n_emit) to decode only a slice"""
        idx_tot = hdr_tot = pcm_tot = 0
        self.descs, self.patch_list = [], []
        lay = []
        for i, s in enumerate(staged_list):
            bl = s.block_len
            n = s.info.blocks * bl
            row_begin, n_emit = (0, s.words) if windows is None else windows[i]
            d = StreamDesc(idx_off=idx_tot, hdr_off=hdr_tot, pcm_off=pcm_tot, n_emit=n_emit,
                           level=s.info.level, rows=s.info.rows, nrows=s.info.blocks * s.info.rows,
                           row_begin=row_begin)
            self.descs.append(d)
            lay.append((idx_tot, hdr_tot, pcm_tot, n, n_emit))
            if s.patches is not None:
                for p in s.patches:
                    self.patch_list.append(Patch(p.sample, p.value, i))
            idx_tot += _round_up(max(n, 1), 64)
            hdr_tot += max(s.info.blocks, 1)
            pcm_tot += _round_up(max(n_emit, 1), 64)
        self.idx = np.zeros(idx_tot, dtype=np.int16)
        self.hdr = np.zeros((hdr_tot, 2), dtype=np.uint32)
        self.pcm_words = pcm_tot
        self.layout = lay
        for s, (io, ho, po, n, ne) in zip(staged_list, lay):
            self.idx[io:io + n] = s.idx[:n]
            self.hdr[ho:ho + s.info.blocks] = s.hdr[:s.info.blocks]
        self.patches = (Patch * len(self.patch_list))(*self.patch_list) if self.patch_list else None


def synth(dev, staged_list, fmt=FMT_S16LE, flags=PLAN_AUTO, windows=None, return_stats=False, patch_subset=None, packed=False, mform=False,
          f32=False, omit=()):
    """Upload staged streams, run the hot path once, return one PCM array (uint16 view of the bytes) per stream.
    patch_subset (tests): keep only these entries of the batch's H1 patch list.
    packed: stage the packed form too (acmhip_pack_tiles) and bind it: whole tiles from row 0 are read from it.
    mform: the same with the byte-plane form (acmhip_mform_rows) and the matrix-core build of the lean kernel.
    f32: acmhip_plan_launch_f32 instead (fmt is ignored): one float32 array per stream.
    omit (tests): streams that keep their place in the three arenas but are left out of the plan's descriptor list; what comes back
    for them is whatever the launch found in their PCM slot."""
    ar = Arena(staged_list, windows)
    if patch_subset is not None and ar.patch_list:
        ar.patch_list = [ar.patch_list[k] for k in patch_subset]
        ar.patches = (Patch * len(ar.patch_list))(*ar.patch_list) if ar.patch_list else None
    d_idx = dev.malloc(ar.idx.nbytes)
    d_hdr = dev.malloc(ar.hdr.nbytes)
    d_pcm = dev.malloc(ar.pcm_words * (4 if f32 else 2))
    try:
        if FILL_MODE:                   # whatever the allocator handed back (the PCM of the synth before, as a rule) is gone before the launch
            dev.memset(d_pcm, 0xFF if f32 else 0xA5, ar.pcm_words * (4 if f32 else 2))
        dev.upload(d_idx, ar.idx)
        dev.upload(d_hdr, ar.hdr)
        pk, pk_ptrs = None, ()
        if packed:
            patched = {p.stream for p in ar.patch_list}
            pk = pack_streams(ar.idx, ar.descs)
            for i in patched:
                pk.streams[i].ntiles = 0
            pk_ptrs = pk.upload(dev)
        elif mform:
            patched = {p.stream for p in ar.patch_list}
            pk = mform_streams(ar.idx, ar.descs)
            for i in patched:
                pk.streams[i].ntiles = 0
            pk_ptrs = pk.upload(dev)
        descs, patches, forms = ar.descs, ar.patches, pk.streams if pk else None
        if omit:
            keep = [i for i in range(len(descs)) if i not in omit]
            at = {i: k for k, i in enumerate(keep)}
            left = [Patch(p.sample, p.value, at[p.stream]) for p in ar.patch_list if p.stream in at]
            descs, patches = [descs[i] for i in keep], (Patch * len(left))(*left) if left else None
            forms = [forms[i] for i in keep] if forms else None
        plan = Plan(dev, descs, patches, flags, packed=forms)
        if pk and mform:
            plan.bind_mform(*pk_ptrs)
        elif pk:
            plan.bind_packed(*pk_ptrs)
        if f32:
            plan.launch_f32(d_idx, d_hdr, d_pcm)
        else:
            plan.launch(d_idx, d_hdr, d_pcm, fmt)
        out = np.zeros(ar.pcm_words, dtype=np.float32 if f32 else np.uint16)
        dev.download(out, d_pcm)
        st = plan.stats()
        plan.destroy()
        for p in pk_ptrs:
            dev.free(p)
    finally:
        dev.free(d_idx)
        dev.free(d_hdr)
        dev.free(d_pcm)
    res = [out[po:po + ne].copy() for (_, _, po, _, ne) in ar.layout]
    return (res, st) if return_stats else res


PARSE_HOST, PARSE_DEVICE, PARSE_AUTO = 0, 1, 2


BATCH_PCM_PINNED = 1
BATCH_STAGE_PACKED = 2
BATCH_STAGE_BYTEPLANE = 4
BATCH_STAGE_INT16 = 8
BATCH_PCM_F32 = 16


class _IndexOut:
    """the marks acm_batch_decode_indexed fills for these items: one allocation, acm_batch_index_blocks() + 1 entries per item"""

    def __init__(self, items, n, force_chans):
        need = np.zeros(max(n, 1), dtype=np.uint64)
        lib().acm_batch_index_blocks(items, n, force_chans, need.ctypes.data)
        self.n = n
        self.at = np.zeros(n + 1, dtype=np.int64)
        self.at[1:] = np.cumsum(need[:n].astype(np.int64) + 1)
        self.marks = np.zeros(int(self.at[n]), dtype=BLOCK_MARK_DT)
        self.out = (BatchIndexOut * max(n, 1))()
        for k in range(n):
            self.out[k].marks = self.marks.ctypes.data + int(self.at[k]) * BLOCK_MARK_DT.itemsize
            self.out[k].max_blocks = int(need[k])

    def result(self):
        """what batch.build_index returns: a BlockIndex per item, an empty one for a file that is not ACM"""
        res = []
        for k in range(self.n):
            o, at = self.out[k], int(self.at[k])
            if o.status != 0:
                res.append(as_index(np.zeros(0, dtype=BLOCK_MARK_DT), None))
            else:
                res.append(as_index(self.marks[at:at + o.blocks + 1].copy(), o.end_status))
        return res


def batch_decode(dev, files, force_chans=0, fmt=FMT_S16LE, threads=0, flags=PLAN_AUTO, parse=PARSE_HOST, pinned=False, prestage=False,
                 packed=False, byteplane=None, index=False, batch_flags=0):
    """acm_batch_decode over a list of bytes objects -> (list of (status, uint16 array), BatchTiming).
    index=True: acm_batch_decode_indexed - the block index of every file, a by-product of the decode's own parse, as a further, last
    element in the form batch.build_index returns.  batch_flags: further ACM_BATCH_* bits (block ranges).

    pinned=True: the output buffers are carved from one pinned arena (acmhip_host_alloc) and the call is told so
    (ACM_BATCH_PCM_PINNED: the read-back engine writes them directly); the arrays returned are copies.
    prestage=True: the bit parsing runs first, on its own (acm_batch_prestage: no device involved), and the decode gets its result.
    packed=True: ACM_BATCH_STAGE_PACKED - the host pool also packs the whole tiles, the upload carries the packed form.
    byteplane: None = the library's default (the byte-plane form wherever a stream can have it: first pass on the matrix cores),
    True = ACM_BATCH_STAGE_BYTEPLANE spelled out, False = ACM_BATCH_STAGE_INT16 (every row staged as int16)."""
    n = len(files)
    bufs = [_as_u8(f) for f in files]
    infos = [probe(b, force_chans) for b in bufs]
    sizes = [i.total_values if rc == 0 else 0 for rc, i in infos]
    arena = C.c_void_p()
    if pinned:
        offs, at = [], 0
        for sz in sizes:
            offs.append(at)
            at += (sz + 63) // 64 * 64
        _check(lib().acmhip_host_alloc(max(at, 1) * 2, C.byref(arena)), "acmhip_host_alloc")
        whole = np.ctypeslib.as_array(C.cast(arena, C.POINTER(C.c_uint16)), shape=(max(at, 1),))
        whole[:] = 0
        outs = [whole[o:o + sz] for o, sz in zip(offs, sizes)]
    else:
        # resident buffers (np.zeros hands out untouched pages: the library's copy-out threads would spend the call
        # taking first-touch page faults, which is the caller's allocation policy, not the decode)
        outs = [np.empty(sz, dtype=np.uint16) for sz in sizes]
        for o in outs:
            o.fill(0)
    items = (BatchItem * max(n, 1))()
    for k in range(n):
        items[k].data = bufs[k].ctypes.data
        items[k].len = bufs[k].size
        items[k].pcm = outs[k].ctypes.data if outs[k].size else None
        items[k].pcm_cap = outs[k].size
    opts = BatchOpts(force_chans, fmt, threads, flags | PLAN_EXTRA, parse, BATCH_EXTRA | batch_flags | (BATCH_PCM_PINNED if pinned else 0) |
                     (BATCH_STAGE_PACKED if packed else 0) | (BATCH_STAGE_BYTEPLANE if byteplane else 0) | (BATCH_STAGE_INT16 if byteplane is False else 0))
    tm = BatchTiming()
    _fill(dev)
    pre = C.c_void_p()
    ix = _IndexOut(items, n, force_chans) if index else None
    try:
        if prestage:
            _check(lib().acm_batch_prestage(items, n, C.byref(opts), C.byref(pre), None), "acm_batch_prestage")
            opts.prestaged = pre
        if ix is not None:
            _check(lib().acm_batch_decode_indexed(dev.h, items, n, C.byref(opts), ix.out, C.byref(tm)), "acm_batch_decode_indexed")
        else:
            _check(lib().acm_batch_decode(dev.h, items, n, C.byref(opts), C.byref(tm)), "acm_batch_decode")
        res = [(items[k].status, outs[k][:items[k].words].copy() if pinned else outs[k][:items[k].words]) for k in range(n)]
    finally:
        if pre:
            lib().acm_batch_prestage_free(pre)
        if pinned:
            del outs, whole
            lib().acmhip_host_free(arena)
    return (res, tm, ix.result()) if ix is not None else (res, tm)


def _batch_items(files):
    bufs = [_as_u8(f) for f in files]
    items = (BatchItem * max(len(files), 1))()
    for k, b in enumerate(bufs):
        items[k].data = b.ctypes.data
        items[k].len = b.size
    return bufs, items


def batch_pcm_words(files, force_chans=0):
    """16-bit words of device memory batch_decode_device needs for these files."""
    bufs, items = _batch_items(files)
    return int(lib().acm_batch_pcm_words(items, len(files), force_chans))


def batch_decode_device(dev, files, d_pcm, d_pcm_words, force_chans=0, fmt=FMT_S16LE, threads=0, flags=PLAN_AUTO,
                        parse=PARSE_AUTO, f32=False, batch_flags=0, index=False):
    """acm_batch_decode with device-resident output: PCM of stream k lands at d_pcm + 2*offsets[k] bytes.
    f32=True: ACM_BATCH_PCM_F32 - float32 samples at d_pcm + 4*offsets[k] bytes (d_pcm_words counts floats then).
    batch_flags: further ACM_BATCH_* bits (staging, block ranges).

    Returns (statuses, words, offsets, BatchTiming); nothing is copied back to the host.  index=True: acm_batch_decode_indexed - the block
    index of every file, in the form batch.build_index returns, as a further, last element."""
    bufs, items = _batch_items(files)
    opts = BatchOpts(force_chans, fmt, threads, flags | PLAN_EXTRA, parse, BATCH_EXTRA | batch_flags | (BATCH_PCM_F32 if f32 else 0),
                     d_pcm, d_pcm_words)
    tm = BatchTiming()
    _fill(dev)
    n = len(files)
    ix = _IndexOut(items, n, force_chans) if index else None
    if ix is not None:
        _check(lib().acm_batch_decode_indexed(dev.h, items, n, C.byref(opts), ix.out, C.byref(tm)), "acm_batch_decode_indexed")
    else:
        _check(lib().acm_batch_decode(dev.h, items, n, C.byref(opts), C.byref(tm)), "acm_batch_decode")
    res = ([int(items[k].status) for k in range(n)], [int(items[k].words) for k in range(n)],
           [int(items[k].dev_off) for k in range(n)], tm)
    return res + (ix.result(),) if ix is not None else res


# --------------------------------------------------------------------------- windows through a block index
def _window_tables(files, index, windows, force_chans=0):
    """items / index / window tables of acm_batch_decode_windows.  index[i]: the marks of files[i] as index_file returns them (an
    empty array or None for a file that is not ACM), or a pair (marks, end_status).  With the marks alone the end status of the
    stream is asked of the host stager: one block past the index.  windows: (file_no, first_word, max_words) triples."""
    bufs, items = _batch_items(files)
    n = len(files)
    keep = []
    ix = (BatchIndex * max(n, 1))()
    for i in range(n):
        e = index[i]
        end = None
        if isinstance(e, tuple):
            e, end = e
        elif isinstance(e, BlockIndex):
            end = e.end_status
        if e is None or len(e) == 0:
            continue
        m = np.ascontiguousarray(np.asarray(e), dtype=BLOCK_MARK_DT)
        keep.append(m)
        if end is None:
            end = _end_status(bufs[i], m, force_chans)
        ix[i].marks = m.ctypes.data
        ix[i].blocks = m.size - 1
        ix[i].end_status = end
    return bufs, items, ix, _windows(windows), keep


def _windows(windows):
    """the acm_batch_window table of (file_no, first_word, max_words) triples"""
    wins = (BatchWindow * max(len(windows), 1))()
    for k, (f, first, count) in enumerate(windows):
        wins[k].item, wins[k].first_word, wins[k].max_words = f, first, count
    return wins


def _end_status(buf, marks, force_chans=0):
    """what ends the stream behind its last indexed block (acm_stage_info.end_status of acm_index_file), from the index alone"""
    rc, st = stage_window(buf, marks, marks.size - 1, 1, force_chans)
    return rc if rc != 0 else st.info.end_status


def batch_window_pcm_words(files, windows, force_chans=0):
    """samples of device memory batch_decode_windows_device needs for these windows at most"""
    bufs, items = _batch_items(files)
    return int(lib().acm_batch_window_pcm_words(items, len(files), _windows(windows), len(windows), force_chans))


def batch_decode_windows(dev, files, index, windows, force_chans=0, fmt=FMT_S16LE, threads=0, flags=PLAN_AUTO, parse=PARSE_HOST, caps=None):
    """acm_batch_decode_windows with host output -> (list of (status, words, uint16 array), WindowTiming).
    caps: per-window capacity of the host buffer (default: max_words); the array holds min(words, cap) samples."""
    bufs, items, ix, wins, keep = _window_tables(files, index, windows, force_chans)
    nw = len(windows)
    outs = []
    for k in range(nw):
        cap = windows[k][2] if caps is None else caps[k]
        o = np.zeros(max(cap, 1), dtype=np.uint16)
        outs.append(o)
        wins[k].pcm = o.ctypes.data
        wins[k].pcm_cap = cap
    opts = BatchOpts(force_chans, fmt, threads, flags | PLAN_EXTRA, parse, 0)
    tm = WindowTiming()
    _fill(dev)
    _check(lib().acm_batch_decode_windows(dev.h, items, len(files), ix, wins, nw, C.byref(opts), C.byref(tm)), "acm_batch_decode_windows")
    return [(int(wins[k].status), int(wins[k].words), outs[k][:min(int(wins[k].words), int(wins[k].pcm_cap))]) for k in range(nw)], tm


def batch_decode_windows_device(dev, files, index, windows, d_pcm, d_pcm_words, force_chans=0, fmt=FMT_S16LE, threads=0, flags=PLAN_AUTO,
                                parse=PARSE_HOST, f32=False):
    """acm_batch_decode_windows with device-resident output: the first requested sample of window k lands at sample offsets[k] of d_pcm
    (int16, or float32 with f32=True).  Returns (statuses, words, offsets, slots, WindowTiming); slots[k] = (slot_off, slot_words), the
    region of d_pcm the call may have written for window k."""
    bufs, items, ix, wins, keep = _window_tables(files, index, windows, force_chans)
    nw = len(windows)
    opts = BatchOpts(force_chans, fmt, threads, flags | PLAN_EXTRA, parse, BATCH_PCM_F32 if f32 else 0, d_pcm, d_pcm_words)
    tm = WindowTiming()
    _fill(dev)
    _check(lib().acm_batch_decode_windows(dev.h, items, len(files), ix, wins, nw, C.byref(opts), C.byref(tm)), "acm_batch_decode_windows")
    return ([int(wins[k].status) for k in range(nw)], [int(wins[k].words) for k in range(nw)], [int(wins[k].dev_off) for k in range(nw)],
            [(int(wins[k].slot_off), int(wins[k].slot_words)) for k in range(nw)], tm)


def batch_decode_windows_dense(dev, files, index, windows, d_pcm, d_pcm_words, frames, channels=1, planar=False, force_chans=0,
                               fmt=FMT_S16LE, threads=0, flags=PLAN_AUTO, parse=PARSE_HOST, f32=False, batch_flags=0, dense_flags=None,
                               check=True, mix=False, rate=None, speeds=None):
    """acm_batch_decode_windows_dense: the windows as len(windows) rows of frames * channels samples in d_pcm (int16, or float32 with
    f32=True), row k at sample k * frames * channels - interleaved, or a plane per channel with planar=True - zeros behind what a window
    delivers.  mix=True (ACM_DENSE_MIX): a window of a file with the other channel count counts that file's own samples and its row is
    converted - stereo averaged into mono, mono repeated in both channels.  rate (ACM_DENSE_RESAMPLE): the batch's sample rate; a window
    of a file at another rate counts that file's own samples and its row is resampled (dense_resampled_frames says to how many frames).
    speeds (ACM_DENSE_SPEED, with rate): (num, den) per window, or None for 1/1 - window k is played at num / den, and a ratio the exact
    filter does not take gets the wide one (dense_speed_frames).
    Returns (statuses, words, WindowTiming).  check=False (tests
    of the refusals): the return code instead of an exception, as a fourth element; dense_flags: the raw acm_dense_opts.flags instead of planar and mix; frames None: no acm_dense_opts at all; dev None: the call's
    own answer to a missing handle."""
    bufs, items, ix, wins, keep = _window_tables(files, index, windows, force_chans)
    nw = len(windows)
    opts, dense = _dense_options(wins, d_pcm, d_pcm_words, frames, channels, planar, force_chans, fmt, threads, flags, parse, f32, batch_flags,
                                 dense_flags, mix, rate, speeds)
    tm = WindowTiming()
    _fill(dev)
    rc = lib().acm_batch_decode_windows_dense(dev.h if dev is not None else None, items, len(files), ix, wins, nw, C.byref(opts),
                                              C.byref(dense) if dense is not None else None, C.byref(tm))
    if check:
        _check(rc, "acm_batch_decode_windows_dense")
    res = ([int(wins[k].status) for k in range(nw)], [int(wins[k].words) for k in range(nw)], tm)
    return res if check else res + (rc,)


def _dense_options(wins, d_pcm, d_pcm_words, frames, channels, planar, force_chans, fmt, threads, flags, parse, f32, batch_flags, dense_flags, mix,
                   rate, speeds):
    """what every call of the dense family begins with, from batch_decode_windows_dense's arguments: the BatchOpts, the DenseOpts (None
    with frames None), and the speeds in wins[k].reserved"""
    opts = BatchOpts(force_chans, fmt, threads, flags | PLAN_EXTRA, parse, batch_flags | (BATCH_PCM_F32 if f32 else 0), d_pcm, d_pcm_words)
    if dense_flags is None:
        dense_flags = (DENSE_PLANAR if planar else 0) | (DENSE_MIX if mix else 0) | (DENSE_RESAMPLE if rate is not None else 0) | \
            (DENSE_SPEED if speeds is not None else 0)
    for k, sp in enumerate(speeds or ()):
        if sp is not None:
            wins[k].reserved = sp[0] << 16 | sp[1]
    return opts, None if frames is None else DenseOpts(frames, channels, dense_flags, rate or 0)


def dense_overlay_gain(energy_a, energy_b, snr):
    """acm_dense_overlay_gain: the Q12 gain of b that makes the power ratio a : b what snr (Q16) asks for, from the rows' sums of squares"""
    return int(lib().acm_dense_overlay_gain(energy_a, energy_b, snr))


def batch_decode_windows_overlay(dev, files, index, windows, rows, d_pcm, d_pcm_words, frames, channels=1, planar=False, force_chans=0,
                                 fmt=FMT_S16LE, threads=0, flags=PLAN_AUTO, parse=PARSE_HOST, f32=False, batch_flags=0, dense_flags=None,
                                 check=True, mix=False, rate=None, speeds=None, nrows=None, result_table=False):
    """acm_batch_decode_windows_overlay: the windows are the SOURCE rows of batch_decode_windows_dense (every argument it has means the
    same), and d_pcm receives len(rows) output rows of frames * channels samples, row r at sample r * frames * channels.  rows: tuples
    (a, b, vol, snr, gain) of acm_overlay_row's inputs - b None for ACM_OVERLAY_NONE - or 6-tuples that end in `reserved`, or an array
    of OVERLAY_ROW_DT records (a large batch: nothing is done row by row here; it is not written into); None for no row table at all
    (tests of the refusals: nrows is then what the call is told).  Returns (statuses, words, offsets, gains, WindowTiming): statuses and words are the windows', offsets their
    (dev_off, slot_off, slot_words), gains (g, energy_a, energy_b) per output row - or, with result_table=True (a million rows), the call's own copy of the row table as
    the library left it, an OVERLAY_ROW_DT array whose gain, energy_a and energy_b fields hold them.  check=False: the return code as a sixth element
    instead of an exception."""
    return _overlay_call("acm_batch_decode_windows_overlay", (), dev, files, index, windows, rows, d_pcm, d_pcm_words, frames, channels=channels,
                         planar=planar, force_chans=force_chans, fmt=fmt, threads=threads, flags=flags, parse=parse, f32=f32, batch_flags=batch_flags,
                         dense_flags=dense_flags, check=check, mix=mix, rate=rate, speeds=speeds, nrows=nrows, result_table=result_table)


def _overlay_call(name, extra, dev, files, index, windows, rows, d_pcm, d_pcm_words, frames, channels=1, planar=False, force_chans=0,
                  fmt=FMT_S16LE, threads=0, flags=PLAN_AUTO, parse=PARSE_HOST, f32=False, batch_flags=0, dense_flags=None, check=True, mix=False,
                  rate=None, speeds=None, nrows=None, result_table=False):
    """one call of the overlay family: the entry point `name` of the library with the pointers `extra` - ctypes structures or None, as
    the entry point takes them between the dense options and the row table.  The rest is batch_decode_windows_overlay's"""
    bufs, items, ix, wins, keep = _window_tables(files, index, windows, force_chans)
    nw = len(windows)
    opts, dense = _dense_options(wins, d_pcm, d_pcm_words, frames, channels, planar, force_chans, fmt, threads, flags, parse, f32, batch_flags,
                                 dense_flags, mix, rate, speeds)
    nr = len(rows) if rows is not None else 0
    if isinstance(rows, np.ndarray):
        table = np.array(rows, dtype=OVERLAY_ROW_DT, ndmin=1)
    else:
        table = np.zeros(max(nr, 1), dtype=OVERLAY_ROW_DT)
        for r in range(nr):
            a, b, vol, snr, gain = rows[r][:5]
            table[r] = (a, OVERLAY_NONE if b is None else b, vol, snr, gain, rows[r][5] if len(rows[r]) > 5 else 0, 0, 0)
    entry = {"acm_batch_decode_windows_overlay": lib().acm_batch_decode_windows_overlay,
             "acm_batch_decode_windows_overlay_fir": lib().acm_batch_decode_windows_overlay_fir,
             "acm_batch_decode_windows_features": lib().acm_batch_decode_windows_features,
             "acm_batch_decode_windows_logmel": lib().acm_batch_decode_windows_logmel}[name]
    tm = WindowTiming()
    _fill(dev)
    rc = entry(dev.h if dev is not None else None, items, len(files), ix, wins, nw, C.byref(opts), C.byref(dense) if dense is not None else None,
               *[C.byref(e) if e is not None else None for e in extra],
               C.cast(table.ctypes.data, C.POINTER(OverlayRow)) if rows is not None else None, nr if nrows is None else nrows, C.byref(tm))
    if check:
        _check(rc, name)
    res = ([int(wins[k].status) for k in range(nw)], [int(wins[k].words) for k in range(nw)],
           [(int(wins[k].dev_off), int(wins[k].slot_off), int(wins[k].slot_words)) for k in range(nw)],
           table[:nr] if result_table else list(zip(table["gain"][:nr].tolist(), table["energy_a"][:nr].tolist(), table["energy_b"][:nr].tolist())),
           tm)
    return res if check else res + (rc,)


def fir_response(taps, delay, shift, reserved=0):
    """(FirResponse, the int16 array it points into) of h = taps (None: a null pointer), d = delay, s = shift"""
    h = None if taps is None else np.ascontiguousarray(taps, dtype="<i2")
    return FirResponse(h.ctypes.data if h is not None and h.size else None, h.size if h is not None else 1, delay, shift, reserved), h


def dense_fir_check(taps, delay, shift, reserved=0, ntaps=None):
    """acm_dense_fir_check: 0 for a response acm_batch_decode_windows_overlay_fir takes, else ERR_ARG.  ntaps (tests): the count the
    library is told instead of len(taps)"""
    r, keep = fir_response(taps, delay, shift, reserved)
    if ntaps is not None:
        r.ntaps = ntaps
    return int(lib().acm_dense_fir_check(C.byref(r)))


def fir_opts(responses, of_window, nresp=None, reserved=0):
    """(FirOpts, what it points into) of responses = [(taps, delay, shift[, reserved])] - or an array of FIR_RESPONSE_DT records that
    point at taps the caller keeps alive - and of_window = a response number or None per window (or a uint32 array, FIR_NONE for None).
    Either may be None for a null pointer; nresp (tests): the count the library is told"""
    keep = []
    table = None
    if isinstance(responses, np.ndarray):
        table = np.ascontiguousarray(responses, dtype=FIR_RESPONSE_DT)
    elif responses is not None:
        table = np.zeros(max(len(responses), 1), dtype=FIR_RESPONSE_DT)
        for p, r in enumerate(responses):
            rec, h = fir_response(*r)
            keep.append(h)
            table[p] = (rec.taps or 0, rec.ntaps, rec.delay, rec.shift, rec.reserved)
    of = None
    if of_window is not None:
        of = of_window if isinstance(of_window, np.ndarray) else np.array([FIR_NONE if p is None else p for p in of_window] or [FIR_NONE], dtype="<u4")
        of = np.ascontiguousarray(of, dtype="<u4")
    n = (len(responses) if responses is not None else 0) if nresp is None else nresp
    o = FirOpts(C.cast(table.ctypes.data, C.POINTER(FirResponse)) if table is not None else None, n, of.ctypes.data if of is not None else None, reserved)
    return o, (table, of, keep)


def batch_decode_windows_overlay_fir(dev, files, index, windows, rows, d_pcm, d_pcm_words, frames, responses=None, of_window=None, nresp=None,
                                     fir_reserved=0, no_fir=False, **kw):
    """acm_batch_decode_windows_overlay_fir: batch_decode_windows_overlay (every other argument and what is returned are its) with
    window k convolved with responses[of_window[k]] - (taps, delay, shift) of include/acm_hip.h - before the rows are made from it;
    of_window[k] None: not filtered.  no_fir: no acm_fir_opts at all; nresp, fir_reserved (tests of the refusals): as fir_opts takes them"""
    o, keep = (None, None) if no_fir else fir_opts(responses, of_window, nresp, fir_reserved)
    return _overlay_call("acm_batch_decode_windows_overlay_fir", (o,), dev, files, index, windows, rows, d_pcm, d_pcm_words, frames, **kw)


def feat_bank(n_fft, hop, n_mels, flags, window, cs, mel_first, mel_count, mel_off, mel_w, reserved=0):
    """(FeatBank, the arrays it points into) of acm_feat_bank's fields; a table given as None is a null pointer"""
    def arr(a, dt):
        return None if a is None else np.ascontiguousarray(a, dtype=dt)
    keep = (arr(window, "<i2"), arr(cs, "<i2"), arr(mel_first, "<u2"), arr(mel_count, "<u2"), arr(mel_off, "<u4"), arr(mel_w, "<u2"))
    # an empty table still needs a pointer: the library reads none of it
    ptr = [None if a is None else (a if a.size else np.zeros(1, a.dtype)) for a in keep]
    return FeatBank(n_fft, hop, n_mels, flags, *[None if a is None else a.ctypes.data for a in ptr], reserved), (keep, ptr)


def feat_bank_check(*args, **kw):
    """acm_feat_bank_check over feat_bank's arguments: 0 for a bank acm_batch_decode_windows_features takes, else ERR_ARG"""
    b, keep = feat_bank(*args, **kw)
    return int(lib().acm_feat_bank_check(C.byref(b)))


def feat_frames(T, n_fft, hop, flags):
    """acm_feat_frames: the frames F of a row of T samples"""
    b = FeatBank(n_fft, hop, 1, flags)
    return int(lib().acm_feat_frames(T, C.byref(b)))


def feat_design(rate, n_fft=512, win_length=None, hop=160, n_mels=80, f_min=0.0, f_max=None, flags=FEAT_CENTER):
    """acm_feat_design -> (window int16 [n_fft], cs int16 [n_fft], mel_first uint16 [n_mels], mel_count, mel_off uint32, mel_w uint16):
    a periodic Hann of win_length (n_fft by default) centred in n_fft, the cosines, HTK mel triangles from f_min to f_max (rate / 2 by
    default).  ValueError for arguments the library does not take"""
    win_length = n_fft if win_length is None else win_length
    f_max = rate / 2.0 if f_max is None else f_max
    L = lib()
    nw = C.c_size_t(0)
    args = (rate, n_fft, win_length, hop, n_mels, float(f_min), float(f_max), flags)
    if L.acm_feat_design(*args, None, None, None, None, None, None, 0, C.byref(nw)) != 0:
        raise ValueError("acm_feat_design: rate %r, n_fft %r, win_length %r, hop %r, n_mels %r, f_min %r, f_max %r, flags %r" % args)
    window, cs = np.zeros(n_fft, "<i2"), np.zeros(n_fft, "<i2")
    first, count, off = np.zeros(n_mels, "<u2"), np.zeros(n_mels, "<u2"), np.zeros(n_mels, "<u4")
    w = np.zeros(max(nw.value, 1), "<u2")
    _check(L.acm_feat_design(*args, window.ctypes.data, cs.ctypes.data, first.ctypes.data, count.ctypes.data, off.ctypes.data, w.ctypes.data,
                             nw.value, C.byref(nw)), "acm_feat_design")
    return window, cs, first, count, off, w[:nw.value]


def feat_log(flags=0, floor_q16=0, mul_q24=1 << 24, offset_q16=0, top_q16=0, reserved=0):
    """FeatLog of acm_feat_log's fields"""
    return FeatLog(flags, floor_q16, mul_q24, offset_q16, top_q16, reserved)


def feat_log_check(bank, log):
    """acm_feat_log_check: 0 for a bank - feat_bank's arguments as a tuple or a dict - and a scale - feat_log's, or None for a null
    pointer - that acm_batch_decode_windows_logmel takes, else ERR_ARG"""
    b, keep = feat_bank(**bank) if isinstance(bank, dict) else feat_bank(*bank)
    g = None if log is None else feat_log(**log) if isinstance(log, dict) else feat_log(*log)
    return int(lib().acm_feat_log_check(C.byref(b), C.byref(g) if g is not None else None))


def batch_decode_windows_features(dev, files, index, windows, rows, d_out, d_out_words, frames, bank, responses=None, of_window=None, no_bank=False,
                                  log=None, **kw):
    """acm_batch_decode_windows_features: batch_decode_windows_overlay_fir (every other argument and what is returned are its; channels
    stays 1) whose int16 rows stay in the handle, d_out receiving the float32 mel features of them, d_out_words float32 elements.
    bank: feat_bank's arguments as a tuple or a dict.  responses None: no acm_fir_opts.  no_bank (tests): a null bank.
    log (batch_decode_windows_logmel): the entry point is acm_batch_decode_windows_logmel and takes this FeatLog, or for False none"""
    o, keep = (None, None) if responses is None else fir_opts(responses, of_window, kw.pop("nresp", None), kw.pop("fir_reserved", 0))
    b, keep_b = (None, None) if no_bank else feat_bank(**bank) if isinstance(bank, dict) else feat_bank(*bank)
    name, extra = ("acm_batch_decode_windows_features", (o, b)) if log is None else ("acm_batch_decode_windows_logmel", (o, b, log or None))
    return _overlay_call(name, extra, dev, files, index, windows, rows, d_out, d_out_words, frames, **kw)


def batch_decode_windows_logmel(dev, files, index, windows, rows, d_out, d_out_words, frames, bank, log, **kw):
    """acm_batch_decode_windows_logmel: batch_decode_windows_features (every other argument and what is returned are its) with d_out
    receiving the logarithm of the features, floored, clamped and scaled by log: feat_log's arguments as a tuple or a dict, or None
    (tests) for a null pointer"""
    g = False if log is None else feat_log(**log) if isinstance(log, dict) else feat_log(*log)
    return batch_decode_windows_features(dev, files, index, windows, rows, d_out, d_out_words, frames, bank, log=g, **kw)


# --------------------------------------------------------------------------- the block index of a batch
def batch_index_files(dev, files, parse=PARSE_AUTO, max_group_bytes=0, force_chans=0, threads=0, max_blocks=None, return_status=False):
    """acm_batch_index_files over a list of file images -> (list of BlockIndex, IndexTiming): entry i is what index_file(files[i])
    returns - the device walks the clean streams (PARSE_DEVICE, or PARSE_AUTO where it pays), the host pool indexes the rest - and an
    empty index for a file that is not ACM (status ACM_ERR_NOT_ACM).  dev: a Device, or None with PARSE_HOST / PARSE_AUTO (the pool only).
    max_blocks (tests): the room per item instead of what acm_batch_index_blocks asks for.  return_status: the per-item return codes as a third
    value."""
    bufs, items = _batch_items(files)
    n = len(files)
    need = np.zeros(max(n, 1), dtype=np.uint64)
    lib().acm_batch_index_blocks(items, n, force_chans, need.ctypes.data)
    if max_blocks is not None:
        need[:n] = max_blocks
    at = np.zeros(n + 1, dtype=np.int64)
    at[1:] = np.cumsum(need[:n].astype(np.int64) + 1)
    marks = np.zeros(int(at[n]), dtype=BLOCK_MARK_DT)
    out = (BatchIndexOut * max(n, 1))()
    for k in range(n):
        out[k].marks = marks.ctypes.data + int(at[k]) * BLOCK_MARK_DT.itemsize
        out[k].max_blocks = int(need[k])
    opts = IndexOpts(force_chans, threads, parse, 0, max_group_bytes)
    tm = IndexTiming()
    _fill(dev)
    _check(lib().acm_batch_index_files(dev.h if dev is not None else None, items, n, out, C.byref(opts), C.byref(tm)), "acm_batch_index_files")
    res = []
    for k in range(n):
        if out[k].status != 0:
            res.append(as_index(np.zeros(0, dtype=BLOCK_MARK_DT), None))
        else:
            res.append(as_index(marks[int(at[k]):int(at[k]) + out[k].blocks + 1].copy(), out[k].end_status))
    return (res, tm, [int(out[k].status) for k in range(n)]) if return_status else (res, tm)
