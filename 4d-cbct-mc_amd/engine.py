"""ctypes binding of the engine's C ABI (`include/mcgpu_amd.h`, built as `libmcgpu_amd.so`).

The product path: there is no CPU fallback -- if the HIP extension is missing, loading fails
loudly.  PyTorch is used only by callers that want device tensors / `torch.distributed`; this
module itself needs no torch.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

MODE_FAST, MODE_COMPAT, MODE_FAST_STATS, MODE_FAST_F64 = 0, 1, 2, 3
_MODES = {"fast": MODE_FAST, "compat": MODE_COMPAT, "stats": MODE_FAST_STATS, "fast64": MODE_FAST_F64, MODE_FAST: MODE_FAST,
          MODE_COMPAT: MODE_COMPAT, MODE_FAST_STATS: MODE_FAST_STATS, MODE_FAST_F64: MODE_FAST_F64}

LIB_PATH = Path(os.environ.get("MCGPU_AMD_LIB", Path(__file__).resolve().parent / "libmcgpu_amd.so"))  # override: A/B builds
EXE_PATH = Path(__file__).resolve().parent / "MC-GPU_v1.3.x"

# every symbol declared in include/mcgpu_amd.h
ABI_SYMBOLS = (
    "mcgpu_abi_version", "mcgpu_knob_table", "mcgpu_last_error", "mcgpu_create", "mcgpu_clone", "mcgpu_destroy", "mcgpu_config_i64", "mcgpu_config_f64",
    "mcgpu_host_table", "mcgpu_projection_file_name", "mcgpu_image_words", "mcgpu_launch_shape", "mcgpu_advance_seed",
    "mcgpu_launch_projection", "mcgpu_launch_projection_w2", "mcgpu_run_projection_w2", "mcgpu_finalize_variance", "mcgpu_finalize_variance_host", "mcgpu_tally_stage_plan", "mcgpu_tally_stage_map", "mcgpu_tally_stage_sub_launch", "mcgpu_id_tickets", "mcgpu_id_next_counter", "mcgpu_scheduler_stats", "mcgpu_scheduler_stats_ex", "mcgpu_last_kernel_ms", "mcgpu_clear_image", "mcgpu_run_projection",
    "mcgpu_write_projection", "mcgpu_format_projection", "mcgpu_write_formatted_projection", "mcgpu_dose_info", "mcgpu_dose_read", "mcgpu_dose_clear", "mcgpu_write_dose_report",
    "mcgpu_finalize_projection", "mcgpu_finalize_projection_host", "mcgpu_stack_create", "mcgpu_stack_append", "mcgpu_stack_write_slice", "mcgpu_stack_finish",
    "mcgpu_stack_read", "mcgpu_normalize_stack", "mcgpu_run_scan", "mcgpu_run_scan_multi", "mcgpu_set_projection_angles", "mcgpu_set_geometry_arrays",
    "mcgpu_warp_volume", "mcgpu_warp_geometry", "mcgpu_map_image", "mcgpu_set_geometry_image",
    "mcgpu_resample_plan", "mcgpu_resample_volume", "mcgpu_set_geometry_image_resampled",
    "mcgpu_correspondence_set", "mcgpu_correspondence_fit", "mcgpu_correspondence_predict", "mcgpu_warp_geometry_signal", "mcgpu_correspondence_clear",
    "mcgpu_write_voxel_file", "mcgpu_write_voxel_binary", "mcgpu_kat_rng", "mcgpu_kat_rng_streams", "mcgpu_microbench", "mcgpu_kat_math", "mcgpu_kat_expf", "mcgpu_kat_f32", "mcgpu_kat_fast64", "mcgpu_kat_scatter", "mcgpu_kat_history", "mcgpu_kat_flight", "mcgpu_kat_tile_records", "mcgpu_fdk_reconstruct", "mcgpu_fdk_reconstruct_motion", "mcgpu_wpc_fit", "mcgpu_forward_project", "mcgpu_forward_project_context", "mcgpu_primary_project", "mcgpu_smooth_planes", "mcgpu_primary_moments", "mcgpu_primary_noisy", "mcgpu_sample_compound_poisson", "mcgpu_sample_gaussian", "mcgpu_rooster4d_reconstruct", "mcgpu_rooster4d_stage", "mcgpu_rooster4d_reconstruct_motion", "mcgpu_rooster4d_motion_stage", "mcgpu_register", "mcgpu_register_stage", "mcgpu_invert_field", "mcgpu_field_residual", "mcgpu_shroud_extract", "mcgpu_shroud_signal", "mcgpu_shroud_rows_device", "mcgpu_speedup_run", "mcgpu_speedup_stage", "mcgpu_speedup_train_create", "mcgpu_speedup_train_step", "mcgpu_speedup_train_gradients", "mcgpu_speedup_train_predict", "mcgpu_speedup_train_get_state", "mcgpu_speedup_train_set_state", "mcgpu_speedup_train_destroy", "mcgpu_speedup_train_stage", "mcgpu_segment_run", "mcgpu_segment_stage", "mcgpu_segment_train_create", "mcgpu_segment_train_step", "mcgpu_segment_train_gradients", "mcgpu_segment_train_predict", "mcgpu_segment_train_get_state", "mcgpu_segment_train_set_state", "mcgpu_segment_train_destroy", "mcgpu_segment_train_stage", "mcgpu_set_fast_schedule", "mcgpu_reload_env_knobs",
    "mcgpu_exchange_shared_bytes", "mcgpu_exchange_card_bytes", "mcgpu_exchange_create", "mcgpu_exchange_card", "mcgpu_exchange_connect",
    "mcgpu_exchange_connect_local", "mcgpu_exchange_probe", "mcgpu_exchange_owner", "mcgpu_exchange_begin", "mcgpu_exchange_submit", "mcgpu_exchange_collect",
    "mcgpu_exchange_stats", "mcgpu_exchange_destroy", "mcgpu_copy_to_host",
    "mcgpu_rccl_create", "mcgpu_rccl_reduce_u64", "mcgpu_rccl_destroy",
)


class ScanOptions(C.Structure):
    """mcgpu_scan_options (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("mode", C.c_int), ("first_projection", C.c_int), ("num_projections", C.c_int),
                ("histories_per_projection", C.c_ulonglong), ("crop_nx", C.c_int), ("write_ascii", C.c_int), ("write_stacks", C.c_int),
                ("output_folder", C.c_char_p), ("air_stack", C.c_char_p), ("air_sigma_y", C.c_double), ("air_sigma_x", C.c_double),
                ("pixel_spacing_x", C.c_double), ("pixel_spacing_y", C.c_double),
                ("shared_stacks", C.POINTER(C.c_void_p)), ("slice_of_projection", C.POINTER(C.c_int)), ("progress", C.c_int),
                ("shard", C.c_int), ("projection_stride", C.c_int), ("projection_phase", C.c_int), ("reduce", C.c_int),
                ("write_variance", C.c_int)]


class ScanReport(C.Structure):
    """mcgpu_scan_report (include/mcgpu_amd.h)."""
    _fields_ = [("projections", C.c_int), ("histories_per_projection", C.c_ulonglong), ("seconds_total", C.c_double),
                ("seconds_kernels", C.c_double), ("seconds_after_last_kernel", C.c_double), ("zero_replacement", C.c_float * 3),
                ("seconds_writer", C.c_double), ("kernel_ms_min", C.c_double), ("kernel_ms_max", C.c_double)]


IMAGE_INT16, IMAGE_FLOAT32 = 0, 1
IMAGE_UINT8 = 2  # the resampler only
RESAMPLE_NEAREST, RESAMPLE_LINEAR = 0, 1
_RESAMPLE_DTYPES = {np.dtype(np.uint8): IMAGE_UINT8, np.dtype(np.int16): IMAGE_INT16, np.dtype(np.float32): IMAGE_FLOAT32}
_INTERPOLATORS = {"nearest": RESAMPLE_NEAREST, "linear": RESAMPLE_LINEAR}


class ImageClass(C.Structure):
    """mcgpu_image_class (include/mcgpu_amd.h): one entry of the 12-class table of the CT -> material mapping."""
    _fields_ = [("material", C.c_int), ("density", C.c_float)]


class ImageMapReport(C.Structure):
    """mcgpu_image_map_report (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("reserved", C.c_uint), ("count", C.c_ulonglong * 12), ("first", C.c_longlong * 12),
                ("unmapped", C.c_ulonglong), ("ms_kernel", C.c_double), ("ms_upload", C.c_double), ("ms_install", C.c_double),
                ("kernel_bytes", C.c_ulonglong)]


class ResampleOptions(C.Structure):
    """mcgpu_resample_options (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("n_in", C.c_int * 3), ("spacing_in", C.c_double * 3), ("spacing_out", C.c_double * 3),
                ("dtype", C.c_int), ("interpolator", C.c_int), ("default_value", C.c_double)]


class ResampleReport(C.Structure):
    """mcgpu_resample_report (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("ms_kernel", C.c_double), ("ms_upload", C.c_double), ("ms_download", C.c_double),
                ("kernel_bytes", C.c_ulonglong)]


class PrimaryOptions(C.Structure):
    """mcgpu_primary_options (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("first_projection", C.c_int), ("n_projections", C.c_int), ("su", C.c_int), ("sv", C.c_int),
                ("energy_points", C.c_int), ("crop_nx", C.c_int)]


class PrimaryReport(C.Structure):
    """mcgpu_primary_report (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("n_materials", C.c_int), ("ms_kernel", C.c_double), ("ms_tables", C.c_double),
                ("solid_angle", C.c_double), ("n_energy_points", C.c_int), ("reserved", C.c_int), ("ms_sample", C.c_double)]


class PrimaryNoisyOptions(C.Structure):
    """mcgpu_primary_noisy_options (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("first_projection", C.c_int), ("n_projections", C.c_int), ("su", C.c_int), ("sv", C.c_int),
                ("energy_points", C.c_int), ("crop_nx", C.c_int), ("reserved", C.c_int), ("histories", C.c_double), ("seed", C.c_ulonglong)]


def knob_table():
    """The engine's environment knobs (csrc/knobs.cpp) as a list of dicts {name, type, scope, default, current, what}."""
    lib = load_library()
    n = lib.mcgpu_knob_table(None, 0)
    buf = C.create_string_buffer(n)
    lib.mcgpu_knob_table(buf, n)
    keys = ("name", "type", "scope", "default", "current", "what")
    return [dict(zip(keys, line.split("\t"))) for line in buf.value.decode().split("\n") if line]


class EngineError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"[{code}] {message}")
        self.code = code
        self.message = message


_lib = None


def load_library(path: Optional[os.PathLike] = None):
    """dlopen the engine and declare the prototypes.  Raises if the library or a symbol is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path else LIB_PATH
    if not p.exists():
        raise ImportError(f"{p} not found: build the HIP engine first (python __graft_entry__.py or make -C 4d-cbct-mc_amd/csrc)")
    lib = C.CDLL(str(p))
    missing = [s for s in ABI_SYMBOLS if not hasattr(lib, s)]
    if missing:
        raise ImportError(f"{p} lacks C-ABI symbols: {missing}")
    vp, cp, ci, cull = C.c_void_p, C.c_char_p, C.c_int, C.c_ulonglong
    lib.mcgpu_last_error.restype = cp
    lib.mcgpu_knob_table.argtypes = [C.c_char_p, C.c_size_t]
    lib.mcgpu_knob_table.restype = C.c_size_t
    lib.mcgpu_create.argtypes = [cp, ci, C.POINTER(vp)]
    lib.mcgpu_clone.argtypes = [vp, ci, C.POINTER(vp)]
    lib.mcgpu_destroy.argtypes = [vp]
    lib.mcgpu_destroy.restype = None
    lib.mcgpu_config_i64.argtypes = [vp, cp, C.POINTER(C.c_longlong)]
    lib.mcgpu_config_f64.argtypes = [vp, cp, C.POINTER(C.c_double)]
    lib.mcgpu_host_table.argtypes = [vp, cp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    lib.mcgpu_projection_file_name.argtypes = [vp, ci, cp, C.c_size_t]
    lib.mcgpu_image_words.argtypes = [vp, C.POINTER(C.c_size_t)]
    lib.mcgpu_launch_shape.argtypes = [cull, ci, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(cull)]
    lib.mcgpu_advance_seed.argtypes = [ci, cull, ci]
    lib.mcgpu_launch_projection.argtypes = [vp, ci, ci, ci, cull, cull, ci, vp, vp]
    lib.mcgpu_launch_projection_w2.argtypes = [vp, ci, ci, ci, cull, cull, ci, vp, vp, vp]
    lib.mcgpu_run_projection_w2.argtypes = [vp, ci, ci, ci, cull, cull, ci, vp, vp, C.POINTER(C.c_double), C.POINTER(cull)]
    lib.mcgpu_finalize_variance.argtypes = [vp, vp, vp, cull, ci, vp, ci, vp]
    lib.mcgpu_finalize_variance_host.argtypes = [vp, vp, vp, cull, ci, vp]
    lib.mcgpu_tally_stage_plan.argtypes = [vp, cull, cull, ci, ci, cull, C.POINTER(cull)]
    lib.mcgpu_tally_stage_map.argtypes = [cull, ci, cull, cull, vp, vp]
    lib.mcgpu_tally_stage_sub_launch.argtypes = [cull, cull, cull, cull, C.POINTER(cull), C.POINTER(cull)]
    lib.mcgpu_id_tickets.argtypes = [cull, ci, cull, cull, vp, vp, C.POINTER(cull)]
    lib.mcgpu_id_next_counter.argtypes = [cull, ci]
    lib.mcgpu_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.mcgpu_scheduler_stats.argtypes = [vp, C.POINTER(cull), ci]
    lib.mcgpu_scheduler_stats_ex.argtypes = [vp, C.POINTER(cull), ci, ci]
    lib.mcgpu_clear_image.argtypes = [vp, vp, vp]
    lib.mcgpu_run_projection.argtypes = [vp, ci, ci, ci, cull, cull, ci, vp, C.POINTER(C.c_double), C.POINTER(cull)]
    lib.mcgpu_write_projection.argtypes = [vp, ci, vp, cull, C.c_double, cp]
    lib.mcgpu_format_projection.argtypes = [vp, vp, cull, ci, vp]
    lib.mcgpu_write_formatted_projection.argtypes = [vp, ci, ci, cull, C.c_double, cp]
    lib.mcgpu_dose_info.argtypes = [vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(C.c_size_t)]
    lib.mcgpu_dose_read.argtypes = [vp, vp, vp]
    lib.mcgpu_dose_clear.argtypes = [vp]
    lib.mcgpu_write_dose_report.argtypes = [vp, vp, vp, cull, C.c_double, cp, C.c_size_t]
    lib.mcgpu_finalize_projection.argtypes = [vp, vp, cull, ci, vp, ci, vp]
    lib.mcgpu_finalize_projection_host.argtypes = [vp, vp, cull, ci, vp]
    lib.mcgpu_stack_create.argtypes = [cp, ci, ci, ci, C.c_double, C.c_double, C.POINTER(vp)]
    lib.mcgpu_stack_append.argtypes = [vp, vp]
    lib.mcgpu_stack_write_slice.argtypes = [vp, ci, vp]
    lib.mcgpu_set_projection_angles.argtypes = [vp, ci, C.POINTER(C.c_float)]
    lib.mcgpu_set_geometry_arrays.argtypes = [vp, C.POINTER(ci), C.POINTER(C.c_float), vp, vp]
    lib.mcgpu_warp_volume.argtypes = [vp, C.POINTER(ci), vp, vp, vp, ci, C.c_float, vp, vp]
    lib.mcgpu_warp_geometry.argtypes = [vp, vp, ci, ci, C.c_float]
    lib.mcgpu_map_image.argtypes = [vp, C.POINTER(ci), vp, ci, C.POINTER(vp), C.POINTER(ImageClass), C.POINTER(C.c_float), vp, vp, C.POINTER(ImageMapReport)]
    lib.mcgpu_set_geometry_image.argtypes = [vp, C.POINTER(ci), C.POINTER(C.c_float), vp, ci, C.POINTER(vp), C.POINTER(ImageClass), C.POINTER(C.c_float), ci,
                                             C.POINTER(ImageMapReport)]
    lib.mcgpu_resample_plan.argtypes = [C.POINTER(ResampleOptions), C.POINTER(ci), vp, vp, vp, vp, vp]
    lib.mcgpu_resample_volume.argtypes = [vp, C.POINTER(ResampleOptions), vp, vp, C.POINTER(ResampleReport)]
    lib.mcgpu_set_geometry_image_resampled.argtypes = [vp, C.POINTER(ci), C.POINTER(C.c_double), C.POINTER(C.c_double), vp, ci, C.POINTER(vp),
                                                       C.POINTER(ImageClass), C.POINTER(C.c_float), ci, C.c_double, C.POINTER(ImageMapReport),
                                                       C.POINTER(ResampleReport)]
    lib.mcgpu_correspondence_set.argtypes = [vp, vp, ci, vp, vp, ci, ci]
    lib.mcgpu_correspondence_fit.argtypes = [vp, C.POINTER(vp), ci, vp, vp, ci, ci, vp, vp]
    lib.mcgpu_correspondence_predict.argtypes = [vp, vp, ci, vp]
    lib.mcgpu_warp_geometry_signal.argtypes = [vp, vp, ci, ci, C.c_float]
    lib.mcgpu_correspondence_clear.argtypes = [vp]
    lib.mcgpu_stack_finish.argtypes = [vp, ci, C.POINTER(C.c_float)]
    lib.mcgpu_stack_read.argtypes = [cp, C.POINTER(ci), vp, C.c_size_t]
    lib.mcgpu_normalize_stack.argtypes = [cp, cp, C.c_double, C.c_double, cp, C.c_double, C.c_double]
    lib.mcgpu_run_scan.argtypes = [vp, C.POINTER(ScanOptions), C.POINTER(ScanReport)]
    lib.mcgpu_run_scan_multi.argtypes = [C.POINTER(vp), ci, C.POINTER(ScanOptions), C.POINTER(ScanReport)]
    lib.mcgpu_write_voxel_file.argtypes = [cp, C.POINTER(ci), C.POINTER(C.c_float), vp, vp, ci]
    lib.mcgpu_write_voxel_binary.argtypes = [cp, C.POINTER(ci), C.POINTER(C.c_float), vp, vp]
    lib.mcgpu_kat_rng.argtypes = [vp, ci, ci, ci, ci, ci, vp]
    lib.mcgpu_microbench.argtypes = [vp, ci, vp, ci]
    lib.mcgpu_kat_rng_streams.argtypes = [vp, ci, C.c_uint, C.c_uint, C.c_ulonglong, vp, ci, ci, vp]
    lib.mcgpu_reload_env_knobs.argtypes = [vp]
    lib.mcgpu_copy_to_host.argtypes = [vp, vp, vp, C.c_size_t, vp]
    lib.mcgpu_exchange_shared_bytes.argtypes = [ci]
    lib.mcgpu_exchange_shared_bytes.restype = C.c_size_t
    lib.mcgpu_exchange_card_bytes.argtypes = [ci]
    lib.mcgpu_exchange_card_bytes.restype = C.c_size_t
    lib.mcgpu_exchange_create.argtypes = [ci, ci, ci, C.c_size_t, ci, vp, C.POINTER(vp)]
    lib.mcgpu_exchange_card.argtypes = [vp, vp, C.c_size_t]
    lib.mcgpu_exchange_connect.argtypes = [vp, ci, vp, C.c_size_t]
    lib.mcgpu_exchange_connect_local.argtypes = [vp, vp]
    lib.mcgpu_exchange_owner.argtypes = [vp, C.c_longlong]
    lib.mcgpu_exchange_probe.argtypes = [vp]
    lib.mcgpu_exchange_begin.argtypes = [vp, C.c_longlong, vp, C.POINTER(vp)]
    lib.mcgpu_exchange_submit.argtypes = [vp, C.c_longlong, vp]
    lib.mcgpu_exchange_collect.argtypes = [vp, C.c_longlong, vp, C.POINTER(vp)]
    lib.mcgpu_exchange_stats.argtypes = [vp, C.POINTER(C.c_double)]
    lib.mcgpu_exchange_destroy.argtypes = [vp]
    lib.mcgpu_exchange_destroy.restype = None
    lib.mcgpu_kat_math.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    lib.mcgpu_kat_expf.argtypes = [vp, ci, vp, vp]
    lib.mcgpu_kat_f32.argtypes = [vp, ci, ci, vp, vp, vp]
    lib.mcgpu_kat_fast64.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp]
    lib.mcgpu_kat_scatter.argtypes = [vp, ci, ci, ci, C.c_uint, C.c_uint, vp, vp, vp, vp, vp]
    lib.mcgpu_kat_history.argtypes = [vp, ci, ci, ci, ci, C.c_uint, vp, vp, vp, vp]
    lib.mcgpu_kat_flight.argtypes = [vp, ci, ci, ci, ci, ci, C.c_uint, vp, vp, vp]
    lib.mcgpu_kat_tile_records.argtypes = [ci, vp, vp]
    lib.mcgpu_primary_project.argtypes = [vp, C.POINTER(PrimaryOptions), vp, C.POINTER(PrimaryReport)]
    lib.mcgpu_smooth_planes.argtypes = [ci, vp, vp, ci, ci, ci, C.c_double, C.c_double, C.POINTER(C.c_double)]
    lib.mcgpu_primary_moments.argtypes = [vp, C.POINTER(PrimaryOptions), vp, C.POINTER(PrimaryReport)]
    lib.mcgpu_primary_noisy.argtypes = [vp, C.POINTER(PrimaryNoisyOptions), vp, C.POINTER(PrimaryReport)]
    lib.mcgpu_sample_compound_poisson.argtypes = [ci, vp, vp, vp, vp, ci, ci, ci, C.c_double, C.c_double, C.c_ulonglong, ci]
    lib.mcgpu_sample_gaussian.argtypes = [ci, vp, vp, vp, ci, ci, ci, C.c_ulonglong, ci]
    if path is None:
        _lib = lib
    return lib


def _check(rc: int):
    if rc != 0:
        raise EngineError(rc, load_library().mcgpu_last_error().decode(errors="replace"))


def launch_shape(histories: int, threads_per_block: int, histories_per_thread: int):
    """(blocks, histories_per_thread, total_histories) of the reference launch (MC-GPU_v1.3.cu:823-841)."""
    b, h, t = C.c_int(), C.c_int(), C.c_ulonglong()
    _check(load_library().mcgpu_launch_shape(int(histories), threads_per_block, histories_per_thread, C.byref(b), C.byref(h), C.byref(t)))
    return b.value, h.value, t.value


def tally_stage_plan(detector_words: int, histories: int, workgroups: int, bins: int = 0, limit: int = 1 << 27, ctx=None) -> dict:
    """Plan of the staged detector tally (csrc/tally_stage.hpp): host arithmetic, no device needed."""
    out = (C.c_ulonglong * 6)()
    _check(load_library().mcgpu_tally_stage_plan(ctx.h if ctx is not None else None, int(detector_words), int(histories), int(workgroups), int(bins), int(limit), out))
    return dict(zip(("bins", "words_per_bin", "bin_pixels", "capacity", "bytes", "sub_launches"), (int(v) for v in out)))


def tally_stage_map(detector_words: int, bins: int = 0, first: int = 0, n: Optional[int] = None):
    """(bin, bin-relative word) of the tally words first .. first+n-1, as uint32 arrays."""
    n = int(detector_words) - int(first) if n is None else int(n)
    b, r = np.empty(n, np.uint32), np.empty(n, np.uint32)
    _check(load_library().mcgpu_tally_stage_map(int(detector_words), int(bins), int(first), n, b.ctypes.data, r.ctypes.data))
    return b, r


def id_tickets(count: int, counter: int, first_ticket: int = 0, n: Optional[int] = None):
    """How a FAST launch of `count` histories deals its ids: (lo, hi, n_tickets) of tickets first_ticket .. first_ticket+n-1 of id
    dispenser `counter` -- ids lo[i] .. hi[i]-1 of the launch as uint64 arrays (lo == hi: exhausted) and the dispenser's non-empty
    tickets; n = None: all of those and one more."""
    lib, total = load_library(), C.c_ulonglong()
    if n is None:
        _check(lib.mcgpu_id_tickets(int(count), int(counter), 0, 0, None, None, C.byref(total)))
        n = total.value + 1 - int(first_ticket)
    lo, hi = np.empty(int(n), np.uint64), np.empty(int(n), np.uint64)
    _check(lib.mcgpu_id_tickets(int(count), int(counter), int(first_ticket), int(n), lo.ctypes.data, hi.ctypes.data, C.byref(total)))
    return lo, hi, total.value


def id_next_counter(mask: int, counter: int) -> int:
    """The id dispenser a wave asks after `counter` when `mask` has a bit for every dispenser reported exhausted (64: none is left)."""
    nxt = load_library().mcgpu_id_next_counter(int(mask), int(counter))
    if nxt < 0:
        raise ValueError(f"id_next_counter: no dispenser {counter}")
    return nxt


def tally_stage_sub_launch(first: int, count: int, limit: int, k: int):
    """(first, count) of sub-launch k of a staged launch."""
    f, c = C.c_ulonglong(), C.c_ulonglong()
    _check(load_library().mcgpu_tally_stage_sub_launch(int(first), int(count), int(limit), int(k), C.byref(f), C.byref(c)))
    return f.value, c.value


def _resample_options(shape, spacing, new_spacing, dtype=IMAGE_INT16, interpolator="linear", default_value=0.0) -> ResampleOptions:
    if interpolator not in _INTERPOLATORS:
        raise ValueError(f"interpolator '{interpolator}': 'linear' or 'nearest'")
    if len(shape) != 3 or len(spacing) != 3 or len(new_spacing) != 3:
        raise ValueError("a 3-D shape and one spacing per array axis are needed")
    return ResampleOptions(C.sizeof(ResampleOptions), (C.c_int * 3)(*map(int, shape)), (C.c_double * 3)(*map(float, spacing)),
                           (C.c_double * 3)(*map(float, new_spacing)), int(dtype), _INTERPOLATORS[interpolator], float(default_value))


def resample_plan(shape, spacing, new_spacing) -> dict:
    """The resampling rule per output index of every axis (mcgpu_resample_plan; csrc/resample.hpp states the rule): host arithmetic, no
    device needed.  {"shape": the resampled shape, "base", "next", "frac", "nearest", "inside": one array per axis}."""
    lib = load_library()
    o = _resample_options(shape, spacing, new_spacing)
    n_out = (C.c_int * 3)()
    _check(lib.mcgpu_resample_plan(C.byref(o), n_out, None, None, None, None, None))
    total = sum(n_out)
    base, nxt, nearest = (np.empty(total, dtype=np.int32) for _ in range(3))
    frac, inside = np.empty(total, dtype=np.float64), np.empty(total, dtype=np.uint8)
    _check(lib.mcgpu_resample_plan(C.byref(o), n_out, base.ctypes.data, nxt.ctypes.data, frac.ctypes.data, nearest.ctypes.data, inside.ctypes.data))
    cuts = np.cumsum(list(n_out))[:-1]
    return {"shape": tuple(n_out), "base": np.split(base, cuts), "next": np.split(nxt, cuts), "frac": np.split(frac, cuts),
            "nearest": np.split(nearest, cuts), "inside": [a.astype(bool) for a in np.split(inside, cuts)]}


def advance_seed(batch_number: int, total_histories: int, seed: int) -> int:
    return load_library().mcgpu_advance_seed(batch_number, int(total_histories), seed)


def write_voxel_file(path, n, spacing_cm, material_zyx: np.ndarray, density_zyx: np.ndarray, gzip: bool = True):
    m = np.ascontiguousarray(material_zyx, dtype=np.uint8)
    d = np.ascontiguousarray(density_zyx, dtype=np.float32)
    assert m.size == d.size == int(n[0]) * int(n[1]) * int(n[2])
    _check(load_library().mcgpu_write_voxel_file(str(path).encode(), (C.c_int * 3)(*map(int, n)), (C.c_float * 3)(*map(float, spacing_cm)),
                                                 m.ctypes.data, d.ctypes.data, int(bool(gzip))))


def write_voxel_binary(path, n, spacing_cm, material_zyx: np.ndarray, density_zyx: np.ndarray):
    """Binary sidecar (`geometry.voxbin`) the engine prefers over the text voxel file of the same stem."""
    m = np.ascontiguousarray(material_zyx, dtype=np.uint8)
    d = np.ascontiguousarray(density_zyx, dtype=np.float32)
    assert m.size == d.size == int(n[0]) * int(n[1]) * int(n[2])
    _check(load_library().mcgpu_write_voxel_binary(str(path).encode(), (C.c_int * 3)(*map(int, n)), (C.c_float * 3)(*map(float, spacing_cm)),
                                                   m.ctypes.data, d.ctypes.data))


def kat_tile_records(indices) -> np.ndarray:
    """Tile records of `indices[n_tiles, 64]` (palette index per voxel of a 4x4x4 tile, negative = padding) as the engine builds them
    (include/mcgpu_amd.h: mcgpu_kat_tile_records): uint32[n_tiles, 4] = entries, code, mask low, mask high."""
    v = np.ascontiguousarray(indices, dtype=np.int16).reshape(-1, 64)
    out = np.zeros((v.shape[0], 4), dtype=np.uint32)
    _check(load_library().mcgpu_kat_tile_records(v.shape[0], v.ctypes.data, out.ctypes.data))
    return out


def voxel_sidecar_path(voxel_file) -> Path:
    s = str(voxel_file)
    for ext in (".gz", ".vox"):
        if s.endswith(ext):
            s = s[: -len(ext)]
    return Path(s + ".voxbin")


class StackWriter:
    """MetaImage float32 stack written plane by plane (the reference's `projections_to_itk` + `sitk.WriteImage`)."""

    def __init__(self, path, nx: int, ny: int, nslices: int, spacing=(0.776, 0.776)):
        self.lib = load_library()
        h = C.c_void_p()
        _check(self.lib.mcgpu_stack_create(str(path).encode(), nx, ny, nslices, float(spacing[0]), float(spacing[1]), C.byref(h)))
        self.h, self.shape = h, (ny, nx)

    def append(self, plane: np.ndarray):
        a = np.ascontiguousarray(plane, dtype=np.float32)
        assert a.shape == self.shape
        _check(self.lib.mcgpu_stack_append(self.h, a.ctypes.data))

    def write_slice(self, k: int, plane: np.ndarray):
        """Random-access write (each slice once; not mixed with append): 4-D scans fill the stack grouped by respiratory state."""
        a = np.ascontiguousarray(plane, dtype=np.float32)
        assert a.shape == self.shape
        _check(self.lib.mcgpu_stack_write_slice(self.h, int(k), a.ctypes.data))

    def finish(self, replace_zeros: bool = True) -> float:
        v = C.c_float()
        h, self.h = self.h, None
        _check(self.lib.mcgpu_stack_finish(h, int(replace_zeros), C.byref(v)))
        return v.value


def stack_read(path) -> np.ndarray:
    """float32 [nslices, ny, nx] of a MetaImage stack written by this engine (or SimpleITK, uncompressed)."""
    lib = load_library()
    dims = (C.c_int * 3)()
    _check(lib.mcgpu_stack_read(str(path).encode(), dims, None, 0))
    out = np.zeros((dims[2], dims[1], dims[0]), dtype=np.float32)
    _check(lib.mcgpu_stack_read(str(path).encode(), dims, out.ctypes.data, out.size))
    return out


def normalize_stack(total_stack, air_stack, out_stack, sigma=(10.0, 10.0), spacing=(0.776, 0.776)):
    """log(gaussian_filter(air, sigma) / total) -> out_stack (cbctmc/mc/projection.py:96-115); sigma None/0 = no filter."""
    sy, sx = (0.0, 0.0) if not sigma else (float(sigma[0]), float(sigma[1]))
    _check(load_library().mcgpu_normalize_stack(str(total_stack).encode(), str(air_stack).encode(), sy, sx, str(out_stack).encode(),
                                                float(spacing[0]), float(spacing[1])))


def smooth_planes(planes: np.ndarray, sigma=(10.0, 10.0), device: int = 0) -> np.ndarray:
    """scipy.ndimage.gaussian_filter(plane, sigma, truncate=4, mode="reflect") of every plane of a float32 array [..., ny, nx], on the
    device (mcgpu_smooth_planes).  sigma = (along y, along x); a sigma of 0 leaves its axis alone, both 0 return the planes bit for bit."""
    a = np.ascontiguousarray(planes, dtype=np.float32)
    if a.ndim < 2:
        raise ValueError("planes of at least two dimensions are needed")
    sy, sx = (0.0, 0.0) if not sigma else (float(sigma[0]), float(sigma[1]))
    out = np.empty_like(a)
    ny, nx = a.shape[-2:]
    _check(load_library().mcgpu_smooth_planes(int(device), a.ctypes.data, out.ctypes.data, int(a.size // (ny * nx)), int(ny), int(nx), sy, sx, None))
    return out


def _sampler_planes(*planes):
    """float32 C-contiguous copies of planes [..., ny, nx] of one shape, and (n_planes, ny, nx)."""
    a = [np.ascontiguousarray(p, dtype=np.float32) for p in planes]
    if a[0].ndim < 2 or any(p.shape != a[0].shape for p in a):
        raise ValueError("planes of one shape with at least two dimensions are needed")
    ny, nx = a[0].shape[-2:]
    return a, (int(a[0].size // (ny * nx)), int(ny), int(nx))


def sample_compound_poisson(m0, m1, m2, histories: float, pixel_area: float, seed: int, first_projection: int = 0, device: int = 0) -> np.ndarray:
    """THE NOISE RULE of csrc/primary_project.hip on moment planes a caller brings (float32 [..., ny, nx]: photons, eV and eV^2 per
    cm^2 and history): a plane with the mean m1 and the variance m2 / (histories x pixel_area), sampled on the device
    (mcgpu_sample_compound_poisson).  pixel_area in cm^2; plane p draws with the counter (x, y, first_projection + p, k)."""
    (a0, a1, a2), (n, ny, nx) = _sampler_planes(m0, m1, m2)
    out = np.empty_like(a0)
    _check(load_library().mcgpu_sample_compound_poisson(int(device), a0.ctypes.data, a1.ctypes.data, a2.ctypes.data, out.ctypes.data, n, ny, nx,
                                                        float(histories), float(pixel_area), int(seed) & (2 ** 64 - 1), int(first_projection)))
    return out


def sample_gaussian(mean, variance, seed: int, first_projection: int = 0, device: int = 0) -> np.ndarray:
    """max(0, mean + sqrt(max(variance, 0)) z) of float32 planes [..., ny, nx] on the device (mcgpu_sample_gaussian), z the normal of
    draw k = 2 of the noise rule at (x, y, first_projection + p)."""
    (a, v), (n, ny, nx) = _sampler_planes(mean, variance)
    out = np.empty_like(a)
    _check(load_library().mcgpu_sample_gaussian(int(device), a.ctypes.data, v.ctypes.data, out.ctypes.data, n, ny, nx, int(seed) & (2 ** 64 - 1),
                                                int(first_projection)))
    return out


EXCHANGE_ROOT0, EXCHANGE_ROTATE, EXCHANGE_LOCAL = 0, 1, 2


class Exchange:
    """One rank's end of the tally exchange between the GPUs of one node (mcgpu_exchange_*, include/mcgpu_amd.h): per step
    `begin` -> launch into the returned buffer -> `submit` -> `collect(previous step)`.

    `shared`: a writable buffer of `Exchange.shared_bytes(world)` zeroed bytes seen by every rank -- an `mmap` of one
    /dev/shm file between processes (`Exchange.open_shared`), a bytearray between contexts of one process."""

    def __init__(self, device: int, rank: int, world: int, words: int, shared, policy: int = EXCHANGE_ROOT0):
        self.lib = load_library()
        self._shared = shared  # keeps the mapping alive
        self._buf = (C.c_char * len(shared)).from_buffer(shared)
        if len(shared) < self.shared_bytes(world):
            raise ValueError("shared region too small")
        h = C.c_void_p()
        _check(self.lib.mcgpu_exchange_create(int(device), int(rank), int(world), int(words), int(policy), C.addressof(self._buf), C.byref(h)))
        self.h, self.rank, self.world, self.words, self.policy = h, rank, world, words, policy

    @staticmethod
    def shared_bytes(world: int) -> int:
        return int(load_library().mcgpu_exchange_shared_bytes(int(world)))

    @staticmethod
    def open_shared(path, world: int, create: bool):
        """Map the host region of an exchange between processes: rank 0 creates (and zeroes) the file BEFORE the others open it.
        The creator replaces whatever sits at `path` with a NEW inode of mode 0600 (O_EXCL | O_NOFOLLOW: a symlink planted in the
        world-writable directory is not followed, and a rank left over from a crashed run on the same port keeps its old inode
        instead of sharing counters with this run)."""
        import mmap
        n = Exchange.shared_bytes(world)
        if create:
            try:
                os.unlink(path)
            except FileNotFoundError:
                pass
            fd = os.open(path, os.O_RDWR | os.O_CREAT | os.O_EXCL | os.O_NOFOLLOW, 0o600)
            os.ftruncate(fd, n)  # zero-filled
        else:
            fd = os.open(path, os.O_RDWR | os.O_NOFOLLOW)
        try:
            return mmap.mmap(fd, n)
        finally:
            os.close(fd)

    def card(self) -> bytes:
        n = int(self.lib.mcgpu_exchange_card_bytes(self.world))
        buf = C.create_string_buffer(n)
        _check(self.lib.mcgpu_exchange_card(self.h, buf, n))
        return buf.raw

    def connect(self, peer: int, card: bytes):
        _check(self.lib.mcgpu_exchange_connect(self.h, int(peer), card, len(card)))

    def connect_local(self, other: "Exchange"):
        _check(self.lib.mcgpu_exchange_connect_local(self.h, other.h))

    def probe(self):
        """One small copy-engine transfer to every connected peer, waited for (before the first step)."""
        _check(self.lib.mcgpu_exchange_probe(self.h))

    def owner(self, step: int) -> int:
        return int(self.lib.mcgpu_exchange_owner(self.h, int(step)))

    def begin(self, step: int, stream: int = 0) -> int:
        p = C.c_void_p()
        _check(self.lib.mcgpu_exchange_begin(self.h, int(step), C.c_void_p(stream), C.byref(p)))
        return p.value

    def submit(self, step: int, stream: int = 0):
        _check(self.lib.mcgpu_exchange_submit(self.h, int(step), C.c_void_p(stream)))

    def collect(self, step: int, stream: int = 0) -> Optional[int]:
        """Device pointer of the complete tally of `step` on its owner (valid until begin(step + 2)), None elsewhere."""
        p = C.c_void_p()
        _check(self.lib.mcgpu_exchange_collect(self.h, int(step), C.c_void_p(stream), C.byref(p)))
        return p.value

    def stats(self) -> dict:
        out = (C.c_double * 6)()
        _check(self.lib.mcgpu_exchange_stats(self.h, out))
        return {"last_push_ms": out[0], "last_add_ms": out[1], "pushes": int(out[2]), "collects": int(out[3]), "host_wait_s": out[4], "bytes_per_push": int(out[5])}

    def close(self):
        if getattr(self, "h", None):
            self.lib.mcgpu_exchange_destroy(self.h)
            self.h = None
            del self._buf

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One loaded simulation (input file + tables), optionally resident on one GPU."""

    def __init__(self, input_path, device: int = 0, _clone_of: "Context" = None):
        self.lib = load_library()
        h = C.c_void_p()
        if _clone_of is not None:
            _check(self.lib.mcgpu_clone(_clone_of.h, int(device), C.byref(h)))
        else:
            _check(self.lib.mcgpu_create(str(input_path).encode(), int(device), C.byref(h)))
        self.h = h
        self.device = device
        self.input_path = str(input_path)
        self._correspondence_model = None  # the CorrespondenceModel resident on this context's device (set_correspondence_model)

    def clone(self, device: int = 0) -> "Context":
        """The same simulation on another device without parsing the input files again (mcgpu_clone)."""
        return Context(self.input_path, device, _clone_of=self)

    # -- lifecycle
    def close(self):
        if getattr(self, "h", None):
            self.lib.mcgpu_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- queries
    def geti(self, key: str) -> int:
        v = C.c_longlong()
        _check(self.lib.mcgpu_config_i64(self.h, key.encode(), C.byref(v)))
        return v.value

    def getf(self, key: str) -> float:
        v = C.c_double()
        _check(self.lib.mcgpu_config_f64(self.h, key.encode(), C.byref(v)))
        return v.value

    def host_table(self, name: str, dtype=np.uint8) -> np.ndarray:
        p, n = C.c_void_p(), C.c_size_t()
        _check(self.lib.mcgpu_host_table(self.h, name.encode(), C.byref(p), C.byref(n)))
        buf = (C.c_char * n.value).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype).copy()

    @property
    def num_projections(self) -> int:
        return self.geti("num_projections")

    @property
    def image_words(self) -> int:
        n = C.c_size_t()
        _check(self.lib.mcgpu_image_words(self.h, C.byref(n)))
        return n.value

    @property
    def detector_shape(self):
        return self.geti("num_pixels_z"), self.geti("num_pixels_x")

    def projection_file_name(self, p: int) -> str:
        buf = C.create_string_buffer(1024)
        _check(self.lib.mcgpu_projection_file_name(self.h, p, buf, 1024))
        return buf.value.decode()

    # -- running
    def launch(self, p: int, image_dev_ptr: int, count: int, mode="fast", seed: Optional[int] = None, first: int = 0,
               hpt: Optional[int] = None, stream: int = 0, w2_dev_ptr: int = 0):
        """Asynchronous launch adding into a caller-owned device buffer (e.g. a torch int64 tensor's data_ptr()).
        `w2_dev_ptr`: a second buffer of the same shape that receives the squared tally weights (mcgpu_launch_projection_w2), 0: none."""
        seed = self.geti("seed") if seed is None else seed
        hpt = self.geti("histories_per_thread") if hpt is None else hpt
        _check(self.lib.mcgpu_launch_projection_w2(self.h, p, _MODES[mode], int(seed), int(first), int(count), int(hpt),
                                                   C.c_void_p(image_dev_ptr), C.c_void_p(w2_dev_ptr or None), C.c_void_p(stream)))

    def clear(self, image_dev_ptr: int, stream: int = 0):
        _check(self.lib.mcgpu_clear_image(self.h, C.c_void_p(image_dev_ptr), C.c_void_p(stream)))

    def download_image(self, image_dev_ptr: int, stream: int = 0) -> np.ndarray:
        """uint64[4, Nz, Nx] copy of a device tally (waits for `stream`)."""
        img = np.zeros(self.image_words, dtype=np.uint64)
        _check(self.lib.mcgpu_copy_to_host(self.h, C.c_void_p(image_dev_ptr), img.ctypes.data, img.nbytes, C.c_void_p(stream)))
        nz, nx = self.detector_shape
        return img.reshape(4, nz, nx)

    def reload_env_knobs(self):
        """Read the MCGPU_* tuning knobs of the environment again (they are otherwise read once, at creation)."""
        _check(self.lib.mcgpu_reload_env_knobs(self.h))

    def scheduler_stats(self, reset: bool = True) -> dict:
        """Counters of "stats"-mode launches (diagnostic build): mean flying lanes per wave iteration etc."""
        out = (C.c_ulonglong * 32)()
        _check(self.lib.mcgpu_scheduler_stats_ex(self.h, out, 32, int(reset)))
        names = ("iterations", "flying_lanes", "compton_rounds", "compton_lanes", "rayleigh_rounds", "rayleigh_lanes", "new_rounds", "new_lanes",
                 "scheduling_points", "take_rounds", "take_lanes", "drain_points", "cycles_compton", "cycles_rayleigh", "cycles_new", "cycles_flight",
                 "compton_angle_lanes", "compton_shell_lanes", "compton_done_lanes", "pool_flyable", "pool_wants_new", "pool_compton", "slots_traded", "lanes_taking_a_step",
                 "iter_with_voxel_load", "voxel_load_lanes", "iter_with_sigma_load", "sigma_load_lanes",
                 "cycles_flight_to_voxel", "cycles_flight_resolve", "cycles_settle", "cycles_sched_point")
        return dict(zip(names, [int(v) for v in out]))

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        _check(self.lib.mcgpu_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    def run_projection(self, p: int, count: int, mode="fast", seed: Optional[int] = None, first: int = 0, hpt: Optional[int] = None):
        """Synchronous: returns (image uint64[4, Nz, Nx], kernel_seconds, histories_done)."""
        seed = self.geti("seed") if seed is None else seed
        hpt = self.geti("histories_per_thread") if hpt is None else hpt
        img = np.zeros(self.image_words, dtype=np.uint64)
        secs, done = C.c_double(), C.c_ulonglong()
        _check(self.lib.mcgpu_run_projection(self.h, p, _MODES[mode], int(seed), int(first), int(count), int(hpt), img.ctypes.data,
                                             C.byref(secs), C.byref(done)))
        nz, nx = self.detector_shape
        return img.reshape(4, nz, nx), secs.value, done.value

    def run_projection_with_variance(self, p: int, count: int, mode="fast", seed: Optional[int] = None, first: int = 0, hpt: Optional[int] = None):
        """Synchronous: returns (image, w2, kernel_seconds, histories_done); w2 uint64[4, Nz, Nx] holds, per tally word, the sum of
        (w >> 10)^2 over the histories that scored w there (mcgpu_run_projection_w2)."""
        seed = self.geti("seed") if seed is None else seed
        hpt = self.geti("histories_per_thread") if hpt is None else hpt
        img = np.zeros(self.image_words, dtype=np.uint64)
        w2 = np.zeros(self.image_words, dtype=np.uint64)
        secs, done = C.c_double(), C.c_ulonglong()
        _check(self.lib.mcgpu_run_projection_w2(self.h, p, _MODES[mode], int(seed), int(first), int(count), int(hpt), img.ctypes.data,
                                                w2.ctypes.data, C.byref(secs), C.byref(done)))
        nz, nx = self.detector_shape
        return img.reshape(4, nz, nx), w2.reshape(4, nz, nx), secs.value, done.value

    def reference_shape(self, histories: Optional[int] = None):
        """(batches, hpt, total_histories) the reference would launch for `histories` (COMPAT mode units)."""
        histories = self.geti("total_histories") if histories is None else histories
        tpb, hpt = self.geti("threads_per_block"), self.geti("histories_per_thread")
        blocks, hpt, total = launch_shape(histories, tpb, hpt)
        return blocks * tpb, hpt, total

    def write_projection(self, p: int, image: np.ndarray, total_histories: int, seconds: float = 0.0, file_name: Optional[str] = None):
        img = np.ascontiguousarray(image, dtype=np.uint64).reshape(-1)
        assert img.size == self.image_words
        _check(self.lib.mcgpu_write_projection(self.h, p, img.ctypes.data, int(total_histories), float(seconds),
                                               file_name.encode() if file_name else None))
        return file_name or self.projection_file_name(p)

    def write_projection_device(self, p: int, image_dev_ptr: int, total_histories: int, seconds: float = 0.0, file_name: Optional[str] = None,
                                slot: int = 0, stream: int = 0):
        """The same file with the data lines formatted on the device from a device tally (mcgpu_format_projection +
        mcgpu_write_formatted_projection); synchronises `stream` in between."""
        _check(self.lib.mcgpu_format_projection(self.h, C.c_void_p(image_dev_ptr), int(total_histories), int(slot), C.c_void_p(stream)))
        import torch
        torch.cuda.synchronize()
        _check(self.lib.mcgpu_write_formatted_projection(self.h, p, int(slot), int(total_histories), float(seconds), file_name.encode() if file_name else None))
        return file_name or self.projection_file_name(p)

    # -- post-processing (cbctmc/mc/projection.py) and the whole-scan pipeline
    def finalize_host(self, image: np.ndarray, total_histories: int, crop_nx: int = 0) -> np.ndarray:
        """float32 [3, Nz, crop] = (total, unscattered, scattered), z flipped -- what the reference's Python gets from the ASCII file."""
        img = np.ascontiguousarray(image, dtype=np.uint64).reshape(-1)
        nz, nx = self.detector_shape
        cx = crop_nx if 0 < crop_nx < nx else nx
        out = np.zeros((3, nz, cx), dtype=np.float32)
        _check(self.lib.mcgpu_finalize_projection_host(self.h, img.ctypes.data, int(total_histories), int(crop_nx), out.ctypes.data))
        return out

    def finalize_device(self, image_dev_ptr: int, total_histories: int, planes_dev_ptr: int, crop_nx: int = 0, clear: bool = False, stream: int = 0):
        _check(self.lib.mcgpu_finalize_projection(self.h, C.c_void_p(image_dev_ptr), int(total_histories), int(crop_nx), C.c_void_p(planes_dev_ptr),
                                                  int(clear), C.c_void_p(stream)))

    def finalize_variance_host(self, image: np.ndarray, w2: np.ndarray, total_histories: int, crop_nx: int = 0) -> np.ndarray:
        """float32 [3, Nz, crop]: the variance of every pixel of finalize_host's planes, from the tally and its squared weights."""
        img = np.ascontiguousarray(image, dtype=np.uint64).reshape(-1)
        sq = np.ascontiguousarray(w2, dtype=np.uint64).reshape(-1)
        assert img.size == self.image_words and sq.size == self.image_words
        nz, nx = self.detector_shape
        cx = crop_nx if 0 < crop_nx < nx else nx
        out = np.zeros((3, nz, cx), dtype=np.float32)
        _check(self.lib.mcgpu_finalize_variance_host(self.h, img.ctypes.data, sq.ctypes.data, int(total_histories), int(crop_nx), out.ctypes.data))
        return out

    def finalize_variance_device(self, image_dev_ptr: int, w2_dev_ptr: int, total_histories: int, planes_dev_ptr: int, crop_nx: int = 0,
                                 clear_w2: bool = False, stream: int = 0):
        _check(self.lib.mcgpu_finalize_variance(self.h, C.c_void_p(image_dev_ptr), C.c_void_p(w2_dev_ptr), int(total_histories), int(crop_nx),
                                                C.c_void_p(planes_dev_ptr), int(clear_w2), C.c_void_p(stream)))

    # -- the ray-traced primary (csrc/primary_project.hip states the rule)
    def primary_scan(self, first_projection: int = 0, n_projections: Optional[int] = None, subsamples=(1, 1), energy_points: int = 2,
                     crop_nx: int = 0):
        """The expectation of the `unscattered` plane of projections first_projection .. + n_projections - 1 (default: to the last) of
        the resident geometry: (float32 [n_projections, nz, crop_nx or nx] in finalize's layout and unit, report dict).
        subsamples = (su, sv): sub-points per pixel along x / z, 1..8; energy_points: Gauss-Legendre points per spectrum bin, 1..4."""
        n = self.num_projections - int(first_projection) if n_projections is None else int(n_projections)
        nz, nx = self.detector_shape
        cx = crop_nx if 0 < crop_nx < nx else nx
        o = PrimaryOptions(C.sizeof(PrimaryOptions), int(first_projection), n, int(subsamples[0]), int(subsamples[1]), int(energy_points), int(crop_nx))
        r = PrimaryReport(C.sizeof(PrimaryReport))
        out = np.zeros((max(n, 1), nz, cx), dtype=np.float32)
        _check(self.lib.mcgpu_primary_project(self.h, C.byref(o), out.ctypes.data, C.byref(r)))
        return out, {"ms_kernel": r.ms_kernel, "ms_tables": r.ms_tables, "solid_angle": r.solid_angle, "n_materials": r.n_materials,
                     "n_energy_points": r.n_energy_points}

    def primary_projection(self, p: int, subsamples=(1, 1), energy_points: int = 2, crop_nx: int = 0):
        """primary_scan of the one projection p: (float32 [nz, crop_nx or nx], report dict)."""
        out, report = self.primary_scan(p, 1, subsamples, energy_points, crop_nx)
        return out[0], report

    # -- its noise: moment planes and a seeded draw (csrc/primary_project.hip: MOMENT PLANES, THE NOISE RULE)
    @property
    def pixel_area(self) -> float:
        """Area of a detector pixel [cm^2]: the `a` of the noise rule."""
        return 1.0 / (self.getf("inv_pixel_size_x") * self.getf("inv_pixel_size_z"))

    def primary_moments_scan(self, first_projection: int = 0, n_projections: Optional[int] = None, subsamples=(1, 1), energy_points: int = 2,
                             crop_nx: int = 0):
        """The moment planes M_0, M_1, M_2 of the `unscattered` plane (photons, eV, eV^2 per cm^2 and history) of projections
        first_projection .. + n_projections - 1, from one traversal: (float32 [n_projections, 3, nz, crop_nx or nx], report dict).
        Plane 1 is primary_scan's, bit for bit.  Arguments as primary_scan."""
        n = self.num_projections - int(first_projection) if n_projections is None else int(n_projections)
        nz, nx = self.detector_shape
        cx = crop_nx if 0 < crop_nx < nx else nx
        o = PrimaryOptions(C.sizeof(PrimaryOptions), int(first_projection), n, int(subsamples[0]), int(subsamples[1]), int(energy_points), int(crop_nx))
        r = PrimaryReport(C.sizeof(PrimaryReport))
        out = np.zeros((max(n, 1), 3, nz, cx), dtype=np.float32)
        _check(self.lib.mcgpu_primary_moments(self.h, C.byref(o), out.ctypes.data, C.byref(r)))
        return out, {"ms_kernel": r.ms_kernel, "ms_tables": r.ms_tables, "solid_angle": r.solid_angle, "n_materials": r.n_materials,
                     "n_energy_points": r.n_energy_points}

    def primary_moments(self, p: int, subsamples=(1, 1), energy_points: int = 2, crop_nx: int = 0):
        """primary_moments_scan of the one projection p: (float32 [3, nz, crop_nx or nx], report dict)."""
        out, report = self.primary_moments_scan(p, 1, subsamples, energy_points, crop_nx)
        return out[0], report

    def primary_noisy_scan(self, histories: float, seed: Optional[int] = None, first_projection: int = 0, n_projections: Optional[int] = None,
                           subsamples=(1, 1), energy_points: int = 2, crop_nx: int = 0):
        """The `unscattered` plane of those projections with the mean and the variance that `histories` histories would give it:
        the moments and the compound Poisson sampler run on the device, only the sampled planes come back: (float32 [n_projections,
        nz, crop_nx or nx], report dict with the `seed` used).  A function of (seed, projection, pixel): the same seed gives the same
        bytes and a scan made in two calls equals one call.  seed=None draws one from os.urandom."""
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
        n = self.num_projections - int(first_projection) if n_projections is None else int(n_projections)
        nz, nx = self.detector_shape
        cx = crop_nx if 0 < crop_nx < nx else nx
        o = PrimaryNoisyOptions(C.sizeof(PrimaryNoisyOptions), int(first_projection), n, int(subsamples[0]), int(subsamples[1]), int(energy_points),
                                int(crop_nx), 0, float(histories), int(seed) & (2 ** 64 - 1))
        r = PrimaryReport(C.sizeof(PrimaryReport))
        out = np.zeros((max(n, 1), nz, cx), dtype=np.float32)
        _check(self.lib.mcgpu_primary_noisy(self.h, C.byref(o), out.ctypes.data, C.byref(r)))
        return out, {"ms_kernel": r.ms_kernel, "ms_tables": r.ms_tables, "ms_sample": r.ms_sample, "solid_angle": r.solid_angle,
                     "n_materials": r.n_materials, "n_energy_points": r.n_energy_points, "seed": int(seed)}

    def primary_noisy_projection(self, p: int, histories: float, seed: Optional[int] = None, subsamples=(1, 1), energy_points: int = 2, crop_nx: int = 0):
        """primary_noisy_scan of the one projection p: (float32 [nz, crop_nx or nx], report dict)."""
        out, report = self.primary_noisy_scan(histories, seed, p, 1, subsamples, energy_points, crop_nx)
        return out[0], report

    # -- 4-D: several (geometry, projection angles) jobs on one resident context (cbctmc/mc/simulation.py:527-710)
    def set_projection_angles(self, angles_deg):
        """Explicit projection angles [deg]; pose 0 stays the input file's (pass the first angle twice like the reference
        and start the scan at first_projection=1)."""
        a = np.ascontiguousarray(angles_deg, dtype=np.float32)
        _check(self.lib.mcgpu_set_projection_angles(self.h, int(a.size), a.ctypes.data_as(C.POINTER(C.c_float))))

    def set_geometry_arrays(self, n, spacing_cm, material_zyx: np.ndarray, density_zyx: np.ndarray):
        """Replace the voxel volume from arrays ([z][y][x]); material tables are rebuilt and everything is uploaded again."""
        m = np.ascontiguousarray(material_zyx, dtype=np.uint8)
        d = np.ascontiguousarray(density_zyx, dtype=np.float32)
        assert m.size == d.size == int(n[0]) * int(n[1]) * int(n[2])
        _check(self.lib.mcgpu_set_geometry_arrays(self.h, (C.c_int * 3)(*map(int, n)), (C.c_float * 3)(*map(float, spacing_cm)),
                                                  m.ctypes.data, d.ctypes.data))
        self._correspondence_model = None  # the device model is built anew: a resident correspondence model goes with the old one

    def set_geometry(self, geometry):
        """An `MCGeometry` of the Python mirror, in the orientation its voxel file would have (geo.py:589-599)."""
        mats, dens, spacing_cm = geometry.mcgpu_arrays()
        nx, ny, nz = mats.shape
        self.set_geometry_arrays((nx, ny, nz), spacing_cm, np.transpose(mats, (2, 1, 0)), np.transpose(dens, (2, 1, 0)))

    # -- CT image + segmentations -> geometry on the device (mcgpu_map_image / mcgpu_set_geometry_image; the rule: DESIGN.md row f8)
    @staticmethod
    def _image_arguments(image, segmentations, table, thresholds):
        """The image as int16 or float32, the eight segmentation pointers in the engine's order, the class table and thresholds."""
        from . import geometry
        img = np.ascontiguousarray(geometry.image_values(image))
        if img.ndim != 3:
            raise ValueError(f"a 3-D image is needed, got shape {img.shape}")
        unknown = set(segmentations) - set(geometry.SEGMENTATION_NAMES)
        if unknown:
            raise ValueError(f"unknown segmentations {sorted(unknown)}; known: {geometry.SEGMENTATION_NAMES}")
        keep, ptrs = [img], (C.c_void_p * 8)()
        for k, name in enumerate(geometry.SEGMENTATION_NAMES):
            seg = segmentations.get(name)
            if seg is None:
                continue
            a = np.asarray(seg)
            a = np.ascontiguousarray(a if a.dtype == np.uint8 else a > 0, dtype=np.uint8)
            if a.shape != img.shape:
                raise ValueError(f"segmentation '{name}' of shape {a.shape}, the image has {img.shape}")
            keep.append(a)
            ptrs[k] = a.ctypes.data
        entries = geometry.image_class_table() if table is None else list(table)
        if len(entries) != 12:
            raise ValueError("the class table has 12 (material number, density) entries")
        tab = (ImageClass * 12)(*[ImageClass(int(m), float(d)) for m, d in entries])
        thr = (C.c_float * 3)(*map(float, geometry.IMAGE_THRESHOLDS if thresholds is None else thresholds))
        return img, ptrs, tab, thr, keep

    @staticmethod
    def _image_report(r: ImageMapReport) -> dict:
        return {"count": [int(v) for v in r.count], "first": [int(v) for v in r.first], "unmapped": int(r.unmapped), "ms_kernel": r.ms_kernel,
                "ms_upload": r.ms_upload, "ms_install": r.ms_install, "kernel_bytes": int(r.kernel_bytes)}

    def map_image(self, image, segmentations: dict, table=None, thresholds=None):
        """(materials uint8, densities float32) of a CT image and its segmentations {name of geometry.SEGMENTATION_NAMES: array},
        mapped on the GPU by the rule of `geometry.MaterialMapperPipeline.execute`, in the image's own layout (any 3-D shape).
        Raises ValueError with the number of unmapped voxels, like the host pipeline.  `self.last_image_report` has the counts."""
        img, ptrs, tab, thr, keep = self._image_arguments(image, segmentations, table, thresholds)
        mats, dens = np.empty(img.shape, dtype=np.uint8), np.empty(img.shape, dtype=np.float32)
        rep = ImageMapReport(struct_size=C.sizeof(ImageMapReport))
        _check(self.lib.mcgpu_map_image(self.h, (C.c_int * 3)(*img.shape[::-1]), img.ctypes.data, IMAGE_FLOAT32 if img.dtype == np.float32 else IMAGE_INT16,
                                        ptrs, tab, thr, mats.ctypes.data, dens.ctypes.data, C.byref(rep)))
        self.last_image_report = self._image_report(rep)
        if rep.unmapped:
            raise ValueError(f"{int(rep.unmapped)} voxels are unmapped: no line of the mapping touches them (a body segmentation is missing)")
        return mats, dens

    def set_geometry_image(self, image, segmentations: dict, frame: str = "geometry", image_spacing=(1.0, 1.0, 1.0), table=None, thresholds=None) -> dict:
        """The context's geometry := the mapped CT image, built on the device (mcgpu_set_geometry_image): the context
        `set_geometry(MCGeometry(*MaterialMapperPipeline.execute(image), image_spacing))` gives, without the host passes.
        frame "geometry": arrays [gx, gy, gz] and `image_spacing` (mm) as an `MCGeometry` has them (the rot90 of the voxel file
        happens on the device); frame "engine": arrays [nz, ny, nx], spacing (x, y, z).  Returns the report (counts per class,
        kernel and host times).  EngineError(-2): unmapped voxels or a class without material file; the context is unchanged."""
        img, ptrs, tab, thr, keep = self._image_arguments(image, segmentations, table, thresholds)
        sp = [float(v) for v in image_spacing]
        if frame == "geometry":
            gx, gy, gz = img.shape
            n, spacing_cm = (gy, gx, gz), (sp[1] / 10.0, sp[0] / 10.0, sp[2] / 10.0)
        elif frame == "engine":
            nz, ny, nx = img.shape
            n, spacing_cm = (nx, ny, nz), (sp[0] / 10.0, sp[1] / 10.0, sp[2] / 10.0)
        else:
            raise ValueError(f"frame '{frame}': 'geometry' or 'engine'")
        rep = ImageMapReport(struct_size=C.sizeof(ImageMapReport))
        rc = self.lib.mcgpu_set_geometry_image(self.h, (C.c_int * 3)(*n), (C.c_float * 3)(*spacing_cm), img.ctypes.data,
                                               IMAGE_FLOAT32 if img.dtype == np.float32 else IMAGE_INT16, ptrs, tab, thr, 1 if frame == "geometry" else 0,
                                               C.byref(rep))
        self.last_image_report = self._image_report(rep)
        _check(rc)
        self._correspondence_model = None  # the device model is built anew
        return self.last_image_report

    # -- image resampling on the device (mcgpu_resample_volume / mcgpu_set_geometry_image_resampled; the rule: DESIGN.md row f12)
    @staticmethod
    def _resample_report(r: ResampleReport) -> dict:
        return {"ms_kernel": r.ms_kernel, "ms_upload": r.ms_upload, "ms_download": r.ms_download, "kernel_bytes": int(r.kernel_bytes)}

    def resample_volume(self, array, spacing, new_spacing, interpolator="linear", default_value=0.0) -> np.ndarray:
        """`array` (3-D; uint8, int16 or float32) at `spacing` -> the same element type at `new_spacing`, one spacing per array axis,
        resampled on the GPU as SimpleITK's Resample does for the reference's `resample_image_spacing` (csrc/resample.hpp states the
        rule).  The lerps of "linear" run along the last array axis first.  `self.last_resample_report` has the times."""
        a = np.ascontiguousarray(array)
        if a.ndim != 3 or a.dtype not in _RESAMPLE_DTYPES:
            raise ValueError(f"a 3-D uint8, int16 or float32 array is needed, got {a.dtype} of shape {a.shape}")
        o = _resample_options(a.shape, spacing, new_spacing, _RESAMPLE_DTYPES[a.dtype], interpolator, default_value)
        n_out = (C.c_int * 3)()
        _check(self.lib.mcgpu_resample_plan(C.byref(o), n_out, None, None, None, None, None))
        out = np.empty(tuple(n_out), dtype=a.dtype)
        rep = ResampleReport(struct_size=C.sizeof(ResampleReport))
        _check(self.lib.mcgpu_resample_volume(self.h, C.byref(o), a.ctypes.data, out.ctypes.data, C.byref(rep)))
        self.last_resample_report = self._resample_report(rep)
        return out

    def set_geometry_image_resampled(self, image, segmentations: dict, spacing, new_spacing, frame: str = "geometry", image_default: float = -1000.0,
                                     table=None, thresholds=None) -> dict:
        """`set_geometry_image` of the image and segmentations resampled from `spacing` to `new_spacing` (mm, one per array axis), all on
        the device (mcgpu_set_geometry_image_resampled): the image linearly with `image_default` outside, the segmentations by nearest
        neighbour with 0 outside, as `MCGeometry.from_image(image_spacing=...)` resamples them.  Returns the mapping's report;
        `self.last_resample_report` has the resampler's.  After an EngineError the context is unchanged."""
        img, ptrs, tab, thr, keep = self._image_arguments(image, segmentations, table, thresholds)
        if frame not in ("geometry", "engine"):
            raise ValueError(f"frame '{frame}': 'geometry' or 'engine'")
        rep, rrep = ImageMapReport(struct_size=C.sizeof(ImageMapReport)), ResampleReport(struct_size=C.sizeof(ResampleReport))
        rc = self.lib.mcgpu_set_geometry_image_resampled(self.h, (C.c_int * 3)(*img.shape), (C.c_double * 3)(*map(float, spacing)),
                                                         (C.c_double * 3)(*map(float, new_spacing)), img.ctypes.data,
                                                         IMAGE_FLOAT32 if img.dtype == np.float32 else IMAGE_INT16, ptrs, tab, thr,
                                                         1 if frame == "geometry" else 0, float(image_default), C.byref(rep), C.byref(rrep))
        self.last_image_report, self.last_resample_report = self._image_report(rep), self._resample_report(rrep)
        _check(rc)
        self._correspondence_model = None  # the device model is built anew
        return self.last_image_report

    def set_geometry_from_image(self, image_filepath, segmenter=None, segmenter_kwargs=None, body_segmentation_filepath=None,
                                bone_segmentation_filepath=None, muscle_segmentation_filepath=None, fat_segmentation_filepath=None,
                                liver_segmentation_filepath=None, stomach_segmentation_filepath=None, lung_segmentation_filepath=None,
                                lung_vessel_segmentation_filepath=None, image_spacing=None) -> dict:
        """`set_geometry(MCGeometry.from_image(..., engine_context=self))` with the same arguments, mapped and installed on the device.
        An `image_spacing` that differs from the file's resamples there too: without a segmenter in one call
        (`set_geometry_image_resampled`: the native files go up, nothing comes back); with one, the image is resampled first
        (`resample_volume`), because the segmenter sees the resampled image, and given files after it."""
        from . import geometry
        paths = dict(body=body_segmentation_filepath, bone=bone_segmentation_filepath, muscle=muscle_segmentation_filepath,
                     fat=fat_segmentation_filepath, liver=liver_segmentation_filepath, stomach=stomach_segmentation_filepath,
                     lung=lung_segmentation_filepath, lung_vessel=lung_vessel_segmentation_filepath)
        if segmenter is None:
            image, spacing, segmentations = geometry.load_image_and_segmentations(image_filepath, **paths)  # at the file's spacing
            if not geometry.spacing_differs(image_spacing, spacing):
                return self.set_geometry_image(image, segmentations, frame="geometry", image_spacing=spacing)
            if image.dtype in (np.int16, np.float32):  # the mapping's own element types; a uint8 CT is resampled as uint8, below
                return self.set_geometry_image_resampled(image, segmentations, spacing, image_spacing, frame="geometry",
                                                         image_default=geometry.IMAGE_DEFAULT_HU)
        image, spacing, segmentations = geometry.load_image_and_segmentations(image_filepath, segmenter=segmenter, image_spacing=image_spacing,
                                                                              engine_context=self, **paths)
        return self.set_geometry_image(image, segmentations, frame="geometry", image_spacing=spacing)

    def warp_geometry(self, displacement: np.ndarray, frame: str = "geometry", default_material: int = 1, default_density: float = 0.0013):
        """The context's geometry := warp(base geometry, displacement) entirely on the device (mcgpu_warp_geometry).
        frame "geometry": displacement [3, gx, gy, gz] in the frame of the MCGeometry arrays (what the reference's
        correspondence model predicts; the rot90 of the voxel file is handled on the device); frame "engine": [3, nz, ny, nx].
        Raises EngineError(-5) when the volume is not a palette volume: fall back to warp_volume + set_geometry."""
        u = np.ascontiguousarray(displacement, dtype=np.float32)
        nx, ny, nz = self.geti("num_voxels_x"), self.geti("num_voxels_y"), self.geti("num_voxels_z")
        want = (3, ny, nx, nz) if frame == "geometry" else (3, nz, ny, nx)
        if u.shape != want:
            raise ValueError(f"displacement of shape {u.shape}, expected {want} for frame '{frame}'")
        _check(self.lib.mcgpu_warp_geometry(self.h, u.ctypes.data, 1 if frame == "geometry" else 0, int(default_material), float(default_density)))

    # -- the correspondence model resident on the device (correspondence.py: CorrespondenceModel; mcgpu_correspondence_*)
    def _field_shape(self, frame: str):
        nx, ny, nz = self.geti("num_voxels_x"), self.geti("num_voxels_y"), self.geti("num_voxels_z")
        return (ny, nx, nz) if frame == "geometry" else (nz, ny, nx)

    def set_correspondence_model(self, model, frame: str = "geometry"):
        """Upload a fitted `CorrespondenceModel` (mean float32 or float64, coefficients float64 [3N, K]); it stays resident until
        `clear_correspondence_model`, another upload, `set_geometry` or `close`.  frame as for `warp_geometry`: the model's
        `spatial_shape` is (gx, gy, gz) for "geometry", (nz, ny, nx) for "engine".  EngineError(-5) when K > 4."""
        if not model.is_fitted:
            raise RuntimeError("Correspondence model is not fitted")
        want = self._field_shape(frame)
        if tuple(model.spatial_shape) != want:
            raise ValueError(f"model of spatial shape {tuple(model.spatial_shape)}, expected {want} for frame '{frame}'")
        n, k = 3 * int(np.prod(want)), int(model.signal_n_dims)
        mean = np.asarray(model.mean_vector_field)
        mean = np.ascontiguousarray(mean, dtype=np.float32 if mean.dtype == np.float32 else np.float64).reshape(-1)
        coef = np.ascontiguousarray(model.coefficients, dtype=np.float64)
        ms = np.ascontiguousarray(model.mean_signal, dtype=np.float64).reshape(-1)
        if mean.size != n or coef.shape != (n, k) or ms.size != k:
            raise ValueError(f"model arrays of shapes {mean.shape}, {coef.shape}, {ms.shape} do not describe {n} elements and {k} signal dimensions")
        self._correspondence_model = None
        _check(self.lib.mcgpu_correspondence_set(self.h, mean.ctypes.data, int(mean.dtype == np.float64), coef.ctypes.data, ms.ctypes.data, k,
                                                 1 if frame == "geometry" else 0))
        self._correspondence_model = model

    def fit_correspondence_model(self, fields, pinv, mean_signal, frame: str = "geometry"):
        """The large part of `CorrespondenceModel.fit` on the device: `fields` [T, 3, *shape] float32 (or T such arrays), `pinv`
        [T, K] the pseudo-inverse of the centred signals -> (mean float32 [3N], coefficients float64 [3N, K]); the model stays
        resident.  EngineError(-5) when K > 4 or T > 64: fit on the host."""
        want = (3,) + self._field_shape(frame)
        fs = [np.ascontiguousarray(f, dtype=np.float32) for f in fields]
        for f in fs:
            if f.shape != want:
                raise ValueError(f"field of shape {f.shape}, expected {want} for frame '{frame}'")
        p = np.ascontiguousarray(pinv, dtype=np.float64)
        ms = np.ascontiguousarray(mean_signal, dtype=np.float64).reshape(-1)
        if p.shape != (len(fs), ms.size):
            raise ValueError(f"pseudo-inverse of shape {p.shape}, expected {(len(fs), ms.size)}")
        n = int(np.prod(want))
        mean, coef = np.empty(n, dtype=np.float32), np.empty((n, ms.size), dtype=np.float64)
        ptrs = (C.c_void_p * len(fs))(*[f.ctypes.data for f in fs])
        self._correspondence_model = None
        _check(self.lib.mcgpu_correspondence_fit(self.h, ptrs, len(fs), p.ctypes.data, ms.ctypes.data, int(ms.size), 1 if frame == "geometry" else 0,
                                                 mean.ctypes.data, coef.ctypes.data))
        return mean, coef

    def predict_field(self, signal, frame: str = "geometry") -> np.ndarray:
        """float32 [3, *shape]: the field of `signal` evaluated from the resident model (`CorrespondenceModel.predict_field32`);
        `frame` names the frame the model was set with (it only shapes the result)."""
        s = np.ascontiguousarray(signal, dtype=np.float64).reshape(-1)
        out = np.empty((3,) + self._field_shape(frame), dtype=np.float32)
        _check(self.lib.mcgpu_correspondence_predict(self.h, s.ctypes.data, int(s.size), out.ctypes.data))
        return out

    def warp_geometry_by_signal(self, signal, default_material: int = 1, default_density: float = 0.0013):
        """`warp_geometry(model.predict_field32(signal))` without the field: evaluated from the resident model inside the warp
        kernel (mcgpu_warp_geometry_signal).  EngineError(-5): no model resident or not a palette volume -- take the host route."""
        s = np.ascontiguousarray(signal, dtype=np.float64).reshape(-1)
        _check(self.lib.mcgpu_warp_geometry_signal(self.h, s.ctypes.data, int(s.size), int(default_material), float(default_density)))

    def clear_correspondence_model(self):
        self._correspondence_model = None
        _check(self.lib.mcgpu_correspondence_clear(self.h))

    def project_forward(self, angles_deg, detector_size=(1024, 768), detector_pixel_spacing=(0.388, 0.388), detector_offset_x=None,
                        detector_offset_y=0.0, source_to_isocenter=None, source_to_detector=None, spacing_iec=None, origin_iec=None):
        """Joseph forward projection of the context's CURRENT geometry (after set_geometry / warp_geometry), read in place on
        the device (mcgpu_forward_project_context): -> (projections [n][nv][nu] float32, report dict).  Same geometry model and
        detector grid as forward_projection.project_forward (RTK geometry; pixel origin -0.5 n spacing, the reference's
        ConstantImageSource).  spacing_iec / origin_iec: the IEC spacing (mm) and origin forward_projection.prepare_image_for_rtk
        gives the same volume (default: the context's voxel size, volume centred)."""
        from . import defaults, forward_projection
        from .reconstruction import create_geometry
        d = defaults.DEFAULTS
        angles = np.atleast_1d(np.asarray(angles_deg, dtype=np.float64))
        geo = create_geometry(0, source_to_isocenter=d.source_to_isocenter_distance if source_to_isocenter is None else source_to_isocenter,
                              source_to_detector=d.source_to_detector_distance if source_to_detector is None else source_to_detector)
        off_x = d.detector_lateral_displacement if detector_offset_x is None else detector_offset_x
        for a in angles:
            geo.add_projection(float(a), off_x, detector_offset_y)
        return forward_projection._project(self.lib, geo, detector_size, detector_pixel_spacing, spacing_iec, origin_iec, context=self.h)

    def warp_volume(self, material_zyx: np.ndarray, density_zyx: np.ndarray, displacement: np.ndarray, default_material: int, default_density: float):
        """Nearest-neighbour warp on the GPU: out[x] = in[rint(x + u(x))]; displacement [3, nz, ny, nx] (x, y, z components, voxels)."""
        m = np.ascontiguousarray(material_zyx, dtype=np.uint8)
        d = np.ascontiguousarray(density_zyx, dtype=np.float32)
        u = np.ascontiguousarray(displacement, dtype=np.float32)
        nz, ny, nx = m.shape
        assert d.shape == m.shape and u.shape == (3, nz, ny, nx)
        mo, do = np.empty_like(m), np.empty_like(d)
        _check(self.lib.mcgpu_warp_volume(self.h, (C.c_int * 3)(nx, ny, nz), m.ctypes.data, d.ctypes.data, u.ctypes.data, int(default_material),
                                          float(default_density), mo.ctypes.data, do.ctypes.data))
        return mo, do

    def run_scan(self, mode="fast", first_projection=0, num_projections=0, histories=0, crop_nx=0, write_ascii=False, write_stacks=True,
                 output_folder=None, air_stack=None, air_sigma=(10.0, 10.0), pixel_spacing=(0.0, 0.0), shared_stacks=None,
                 slice_of_projection=None, peers=(), shard="histories", projection_stride=0, projection_phase=0, reduce="auto", write_variance=False) -> dict:
        """The whole projection loop as a device/host pipeline (mcgpu_run_scan); returns the timing report.
        `shared_stacks` = three open StackWriters (total, unscattered, scattered) filled by slice index (4-D scans).
        `peers` + shard="histories": the reference's split (tallies summed through the exchange); shard="projections": every
        context simulates whole projections, nothing crosses between devices (SURVEY 8e fallback).  reduce="rccl": the tallies of the
        peers are summed with one ncclReduce per projection instead of the exchange (then projection sharding if RCCL cannot be set up).
        `write_variance` (with write_stacks, one context): also projections_{total,unscattered,scattered}_variance.mha, the per-pixel
        variance of the stacks from the squared weights tallied in the same run."""
        o = ScanOptions()
        o.struct_size = C.sizeof(ScanOptions)
        o.shard = {"histories": 0, "projections": 1}[shard]
        o.reduce = {"auto": 0, "rccl": 1}[reduce]
        o.projection_stride, o.projection_phase = int(projection_stride), int(projection_phase)
        if shared_stacks is not None:
            self._keep = ((C.c_void_p * 3)(*[s.h for s in shared_stacks]), (C.c_int * len(slice_of_projection))(*map(int, slice_of_projection)))
            o.shared_stacks, o.slice_of_projection = self._keep[0], self._keep[1]
        o.mode, o.first_projection, o.num_projections = _MODES[mode], int(first_projection), int(num_projections)
        o.histories_per_projection, o.crop_nx = int(histories), int(crop_nx)
        o.write_ascii, o.write_stacks, o.write_variance = int(bool(write_ascii)), int(bool(write_stacks)), int(bool(write_variance))
        o.output_folder = str(output_folder).encode() if output_folder else None
        o.air_stack = str(air_stack).encode() if air_stack else None
        o.air_sigma_y, o.air_sigma_x = (float(air_sigma[0]), float(air_sigma[1])) if air_sigma else (0.0, 0.0)
        o.pixel_spacing_x, o.pixel_spacing_y = float(pixel_spacing[0]), float(pixel_spacing[1])
        r = ScanReport()
        if peers:  # contexts of the same input on other devices: histories sharded, tallies reduced on this context's device
            hs = (C.c_void_p * (1 + len(peers)))(self.h, *[p.h for p in peers])
            _check(self.lib.mcgpu_run_scan_multi(hs, 1 + len(peers), C.byref(o), C.byref(r)))
        else:
            _check(self.lib.mcgpu_run_scan(self.h, C.byref(o), C.byref(r)))
        return {"projections": r.projections, "histories_per_projection": r.histories_per_projection, "seconds_total": r.seconds_total,
                "seconds_kernels": r.seconds_kernels, "seconds_after_last_kernel": r.seconds_after_last_kernel,
                "seconds_writer": r.seconds_writer, "zero_replacement": [float(v) for v in r.zero_replacement],
                "kernel_ms_min": r.kernel_ms_min, "kernel_ms_max": r.kernel_ms_max}

    # -- dose tallies (SECTION DOSE DEPOSITION of the input file)
    def dose_info(self):
        """(flags, roi6, roi_shape_zyx): flags bit 0 = material tally, bit 1 = voxel tally."""
        flags, roi, n = C.c_int(), (C.c_int * 6)(), C.c_size_t()
        _check(self.lib.mcgpu_dose_info(self.h, C.byref(flags), roi, C.byref(n)))
        r = list(roi)
        shape = (r[5] - r[4] + 1, r[3] - r[2] + 1, r[1] - r[0] + 1) if flags.value & 2 else (0, 0, 0)
        return flags.value, r, shape

    def dose_read(self):
        """(voxels uint64[Dz, Dy, Dx, 2] or None, materials uint64[25, 2] or None) accumulated on the device so far."""
        flags, _, shape = self.dose_info()
        vox = np.zeros(shape + (2,), dtype=np.uint64) if flags & 2 else None
        mat = np.zeros((25, 2), dtype=np.uint64) if flags & 1 else None
        _check(self.lib.mcgpu_dose_read(self.h, vox.ctypes.data if vox is not None else None, mat.ctypes.data if mat is not None else None))
        return vox, mat

    def dose_clear(self):
        _check(self.lib.mcgpu_dose_clear(self.h))

    def write_dose_report(self, voxels, materials, histories_per_projection: int, seconds: float = 0.0) -> str:
        """Writes the voxel dose files (when `voxels` is given) and returns the text of both reports."""
        v = np.ascontiguousarray(voxels, dtype=np.uint64) if voxels is not None else None
        m = np.ascontiguousarray(materials, dtype=np.uint64) if materials is not None else None
        log = C.create_string_buffer(1 << 16)
        _check(self.lib.mcgpu_write_dose_report(self.h, v.ctypes.data if v is not None else None, m.ctypes.data if m is not None else None,
                                                int(histories_per_projection), float(seconds), log, len(log)))
        return log.value.decode(errors="replace")

    def run_all(self, mode="fast", write_projections=True, histories: Optional[int] = None):
        """The projection loop of main() (MC-GPU_v1.3.cu:667-1056) on this context's GPU."""
        out = []
        seed = self.geti("seed")
        histories = self.geti("total_histories") if histories is None else histories
        for p in range(self.num_projections):
            if _MODES[mode] == MODE_COMPAT:
                batches, hpt, total = self.reference_shape(histories)
                img, secs, done = self.run_projection(p, batches, mode, seed=seed, hpt=hpt)
                seed = advance_seed(1, total, seed)
            else:
                img, secs, done = self.run_projection(p, histories, mode, seed=seed)
            name = self.write_projection(p, img, done, secs) if write_projections else None
            out.append((name, img, secs, done))
        return out

    def microbench(self, kind: str):
        """Hardware ceilings measured on this context's device (include/mcgpu_amd.h: mcgpu_microbench): kind "valu_issue" ->
        wave-instructions per ns and SIMD {64 lanes, lanes 0-31, 32 lanes spread}; "atomic_rate" -> scattered 64-bit adds per second;
        "copy_rate" -> bytes read + written per second by a streaming copy."""
        out = (C.c_double * 3)()
        _check(self.lib.mcgpu_microbench(self.h, {"valu_issue": 0, "atomic_rate": 1, "copy_rate": 2}[kind], out, 3))
        return [float(v) for v in out] if kind == "valu_issue" else float(out[0])

    # -- known-answer hooks
    def kat_rng(self, mode, seed: int, batch: int, hpt: int, n: int) -> np.ndarray:
        out = np.zeros(n, dtype=np.float32)
        _check(self.lib.mcgpu_kat_rng(self.h, _MODES[mode], seed, batch, hpt, n, out.ctypes.data))
        return out

    def kat_rng_streams(self, seed: int, projection: int, n_draws: int, first_id: int = 0, n_ids: int = 0, ids=None, generator: int = 0) -> np.ndarray:
        """uint32[n_ids, n_draws]: raw outputs of the FAST per-history streams (generator 1: the Philox-per-draw yardstick)."""
        if ids is not None:
            ids = np.ascontiguousarray(ids, dtype=np.uint64)
            n_ids = ids.size
        out = np.zeros((n_ids, n_draws), dtype=np.uint32)
        _check(self.lib.mcgpu_kat_rng_streams(self.h, generator, seed, projection, first_id, ids.ctypes.data if ids is not None else None,
                                              n_ids, n_draws, out.ctypes.data))
        return out

    def kat_math(self, x: Sequence[float]):
        x = np.ascontiguousarray(x, dtype=np.float64)
        outs = [np.zeros_like(x) for _ in range(4)]
        _check(self.lib.mcgpu_kat_math(self.h, x.size, x.ctypes.data, *[o.ctypes.data for o in outs]))
        return outs

    def kat_fast64(self, u, a, b, c, directions):
        """float64[n, 8] of mcgpu_kat_fast64: sin, cos, 1/sqrt(a), sqrt(a/b), cdt1, rotated direction (3)."""
        u = np.ascontiguousarray(u, dtype=np.uint32)
        a, b, c = (np.ascontiguousarray(v, dtype=np.float64) for v in (a, b, c))
        d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
        assert u.size == a.size == b.size == c.size == d.shape[0]
        out = np.zeros((u.size, 8), dtype=np.float64)
        _check(self.lib.mcgpu_kat_fast64(self.h, u.size, u.ctypes.data, a.ctypes.data, b.ctypes.data, c.ctypes.data, d.ctypes.data, out.ctypes.data))
        return out

    def kat_scatter(self, mode, kind: str, directions, values, ids, materials=None, seed: int = 0, stream_key: int = 0):
        """The FAST scattering samplers as the photon kernels run them (include/mcgpu_amd.h: mcgpu_kat_scatter), one event per item.
        kind "rayleigh" / "compton": values = photon energies [eV], ids = history ids, materials = material numbers - 1;
        kind "rotate" (mode "fast"): values = 1 - cos(theta), ids = the azimuth's 32-bit deviates.
        Returns (energy float32[n], direction float32[n, 3], service calls, final phase, generator state uint32[n, 2])."""
        d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
        n = d.shape[0]
        in4 = np.empty((n, 4), dtype=np.float32)
        in4[:, :3] = d
        in4[:, 3] = np.broadcast_to(np.asarray(values, dtype=np.float32), (n,))
        u64 = np.ascontiguousarray(np.broadcast_to(np.asarray(ids, dtype=np.uint64), (n,)))
        mat = None if materials is None else np.ascontiguousarray(np.broadcast_to(np.asarray(materials, dtype=np.int32), (n,)))
        out4, out_u4 = np.zeros((n, 4), dtype=np.float32), np.zeros((n, 4), dtype=np.uint32)
        _check(self.lib.mcgpu_kat_scatter(self.h, _MODES[mode], {"rotate": 0, "rayleigh": 1, "compton": 2}[kind], n, int(seed), int(stream_key),
                                          in4.ctypes.data, u64.ctypes.data, None if mat is None else mat.ctypes.data, out4.ctypes.data,
                                          out_u4.ctypes.data))
        return out4[:, 0].copy(), out4[:, 1:].copy(), out_u4[:, 0].copy(), out_u4[:, 1].copy(), out_u4[:, 2:].copy()

    def kat_history(self, mode, kind: str, projection: int, items=None, ids=None, seed: int = 0):
        """The two ends of a FAST history as the photon kernels run them (include/mcgpu_amd.h: mcgpu_kat_history), one item per thread,
        under the pose of `projection`.  kind "source": ids = history ids; "tally": items = float32[n, 8] {x, y, z, u, v, w, E, scatter
        state}; "hop": items = {x, y, z, u, v, w, E, -} and ids.  Returns a dict: energy float32[n], direction and position float32[n, 3],
        mfpW, and phase, index, mc, scatter, state uint32[n, 2], word (int64, -1: none), value."""
        in8 = None if items is None else np.ascontiguousarray(items, dtype=np.float32).reshape(-1, 8)
        u64 = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        if kind not in ("source", "tally", "hop"):
            raise ValueError(f"kind '{kind}': 'source', 'tally' or 'hop'")
        if (kind != "source" and in8 is None) or (kind != "tally" and u64 is None):
            raise ValueError(f"kind '{kind}' needs " + ("ids" if kind == "source" else "items" if kind == "tally" else "items and ids"))
        n = in8.shape[0] if in8 is not None else u64.size
        if (in8 is not None and in8.shape[0] != n) or (u64 is not None and u64.size != n) or n == 0:
            raise ValueError("items and ids must hold the same, non-zero, number of entries")
        out8, out_u8 = np.zeros((n, 8), dtype=np.float32), np.zeros((n, 8), dtype=np.uint32)
        _check(self.lib.mcgpu_kat_history(self.h, _MODES[mode], {"source": 0, "tally": 1, "hop": 2}[kind], int(projection), n, int(seed),
                                          None if in8 is None else in8.ctypes.data, None if u64 is None else u64.ctypes.data,
                                          out8.ctypes.data, out_u8.ctypes.data))
        return dict(e=out8[:, 0].copy(), d=out8[:, 1:4].copy(), pos=out8[:, 4:7].copy(), mfpw=out8[:, 7].copy(),
                    phase=out_u8[:, 0].astype(np.int64), index=out_u8[:, 1].astype(np.int64), mc=out_u8[:, 2].astype(np.int64),
                    scatter=out_u8[:, 3].astype(np.int64), state=out_u8[:, 4:6].copy(), word=out_u8[:, 6].view(np.int32).astype(np.int64),
                    value=out_u8[:, 7].astype(np.int64))

    def kat_flight(self, mode, kind: str, projection: int, items, ids=None, max_steps: int = 1, seed: int = 0):
        """The Woodcock flight step of a FAST history as the photon kernels run it (include/mcgpu_amd.h: mcgpu_kat_flight), one item per
        thread, in the kernel variant this context's launches take.  kind "lookup": items = float32[n, 3] points; returns a dict density
        (float32), mc, code, raw, out, exterior, variant.  kind "flight": items = float32[n, 7 or 8] {x, y, z, u, v, w, E}, ids = history
        ids, max_steps in 1..32; returns a dict of the trace -- pos float32[n, max_steps, 3], phase, mc, aux_bits, state uint32[n,
        max_steps, 2] (rows of steps not taken are zero) -- and of the end: final, steps, index, mfpw (float32), end_state, variant, mc_old
        (the material whose cross section is cached, -1: none)."""
        if kind not in ("lookup", "flight"):
            raise ValueError(f"kind '{kind}': 'lookup' or 'flight'")
        it = np.ascontiguousarray(items, dtype=np.float32)
        it = it.reshape(-1, it.shape[-1]) if it.ndim > 1 else it.reshape(-1, 3 if kind == "lookup" else 7)
        n = it.shape[0]
        in8 = np.zeros((n, 8), dtype=np.float32)
        in8[:, :min(it.shape[1], 8)] = it[:, :8]
        u64 = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        if kind == "flight" and (u64 is None or u64.size != n):
            raise ValueError("kind 'flight' needs one id per item")
        rows = int(max_steps) + 1 if kind == "flight" else 1
        out = np.zeros((max(n, 1), max(rows, 1), 8), dtype=np.uint32)
        _check(self.lib.mcgpu_kat_flight(self.h, _MODES[mode], {"lookup": 0, "flight": 1}[kind], int(projection), n, int(max_steps), int(seed),
                                         in8.ctypes.data, None if u64 is None else u64.ctypes.data, out.ctypes.data))
        if kind == "lookup":
            o = out[:, 0]
            return dict(density=o[:, 0].copy().view(np.float32), mc=o[:, 1].astype(np.int64), code=o[:, 2].astype(np.int64), raw=o[:, 3].astype(np.int64),
                        out=o[:, 4] != 0, exterior=o[:, 5] != 0, variant=o[:, 6].astype(np.int64))
        t, e = out[:, :-1], out[:, -1]
        return dict(pos=np.ascontiguousarray(t[:, :, :3]).view(np.float32), phase=t[:, :, 3].astype(np.int64), mc=t[:, :, 4].astype(np.int64),
                    aux_bits=t[:, :, 5].copy(), state=t[:, :, 6:8].copy(), final=e[:, 0].astype(np.int64), steps=e[:, 1].astype(np.int64),
                    index=e[:, 2].astype(np.int64), mfpw=e[:, 3].copy().view(np.float32), end_state=e[:, 4:6].copy(), variant=e[:, 6].astype(np.int64),
                    mc_old=e[:, 7].copy().view(np.int32).astype(np.int64))

    def kat_f32(self, op: int, a, b=None, c=None):
        """Float operations of the COMPAT kernel (include/mcgpu_amd.h: mcgpu_kat_f32)."""
        a = np.ascontiguousarray(a, dtype=np.float32)
        b = np.ascontiguousarray(a if b is None else b, dtype=np.float32)
        out = np.ascontiguousarray(np.zeros_like(a) if c is None else c, dtype=np.float32).copy()
        _check(self.lib.mcgpu_kat_f32(self.h, int(op), a.size, a.ctypes.data, b.ctypes.data, out.ctypes.data))
        return out

    def kat_expf(self, x: Sequence[float]):
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.zeros_like(x)
        _check(self.lib.mcgpu_kat_expf(self.h, x.size, x.ctypes.data, out.ctypes.data))
        return out


def create(input_path, device: int = 0) -> Context:
    return Context(input_path, device)
