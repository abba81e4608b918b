"""ctypes binding of include/fri_hip.h. Plumbing only -- every compute call goes to libfri_hip.so."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# FRI_HIP_LIBRARY: path of an alternative build of the same library (kernel experiments); default = the in-tree build
_SO = os.environ.get("FRI_HIP_LIBRARY") or os.path.join(_HERE, "libfri_hip.so")
NONE = -(2 ** 31)

# every symbol include/fri_hip.h declares (tests/test_abi_symbols.py checks the header against this list)
SYMBOLS = [
    "fri_hip_strerror", "fri_hip_version", "fri_hip_ctx_create", "fri_hip_ctx_destroy", "fri_hip_backend",
    "fri_hip_last_hip_error", "fri_hip_plan_create", "fri_hip_plan_destroy", "fri_hip_plan_num_cells",
    "fri_hip_plan_num_bfs_cells", "fri_hip_plan_num_interior_cells", "fri_hip_plan_coef_count", "fri_hip_plan_pixel_bytes",
    "fri_hip_plan_centers", "fri_hip_plan_valid_mask", "fri_hip_plan_num_some", "fri_hip_plan_neighbour_cells",
    "fri_hip_plan_neighbour_table", "fri_hip_plan_tiling", "fri_hip_plan_tile_table", "fri_hip_transform_quant", "fri_hip_transform_quant_dev",
    "fri_hip_transform_quant_batch_dev", "fri_hip_transform_quant_batch", "fri_hip_predict_histogram",
    "fri_hip_predict_histogram_dev", "fri_hip_fit_value_sums", "fri_hip_fit_value_sums_dev", "fri_hip_fit_width_sums",
    "fri_hip_fit_width_sums_dev", "fri_hip_inverse_transform", "fri_hip_inverse_transform_dev",
    "fri_hip_time_transform_quant_dev", "fri_hip_plan_read_trace", "fri_hip_plan_inverse_lists",
    "fri_hip_shard_size", "fri_hip_shard_image", "fri_hip_multi_create", "fri_hip_multi_destroy", "fri_hip_multi_num_devices",
    "fri_hip_multi_plan", "fri_hip_multi_transform_quant", "fri_hip_predict_histogram_batch_dev", "fri_hip_fit_value_sums_batch_dev",
    "fri_hip_fit_width_sums_batch_dev", "fri_hip_solve6", "fri_hip_fit_value_params", "fri_hip_fit_width_params", "fri_hip_encode_image",
    "fri_hip_encode_image_dev", "fri_hip_inverse_transform_batch_dev", "fri_hip_predict_image", "fri_hip_predict_image_dev",
    "fri_hip_fit_params_batch_dev", "fri_hip_encode_image_batch_dev", "fri_hip_fit_value_params_batch_dev", "fri_hip_fit_width_params_batch_dev",
    "fri_hip_plan_assume_forward_coefficients", "fri_hip_encode_image_batch", "fri_hip_multi_encode_image",
    "fri_hip_plan_set_stream_order", "fri_hip_symbol_stream_batch_dev", "fri_hip_encode_image_symbols", "fri_hip_encode_symbols_batch_dev",
    "fri_hip_plan_set_dequantiser", "fri_hip_plan_tune_forward", "fri_hip_time_transform_quant_streams_dev",
    "fri_hip_plan_set_colour_transform", "fri_hip_quality_matrix", "fri_hip_measure_distortion_dev", "fri_hip_search_quality",
    "fri_hip_search_quality_dev", "fri_hip_estimate_size_dev", "fri_hip_estimate_size", "fri_hip_search_quality_for_size",
    "fri_hip_search_quality_for_size_dev", "fri_hip_plan_predict_grid", "fri_hip_plan_pred_slots", "fri_hip_measure_ssim_dev", "fri_hip_measure_ssim", "fri_hip_search_quality_ssim",
    "fri_hip_search_quality_ssim_dev",
    "fri_hip_plan420_create", "fri_hip_plan420_destroy", "fri_hip_plan420_luma", "fri_hip_plan420_chroma", "fri_hip_split420_dev", "fri_hip_merge420_dev",
    "fri_hip_measure_distortion420_dev", "fri_hip_encode_image420_symbols", "fri_hip_decode_image420", "fri_hip_search_quality420", "fri_hip_search_quality420_dev",
    "fri_hip_search_quality_for_size420", "fri_hip_search_quality_for_size420_dev", "fri_hip_search_quality_ssim420", "fri_hip_search_quality_ssim420_dev",
    "fri_hip_plan_rgba_create", "fri_hip_plan_rgba_destroy", "fri_hip_plan_rgba_colour", "fri_hip_plan_rgba_alpha", "fri_hip_split_rgba_dev", "fri_hip_merge_rgba_dev",
    "fri_hip_encode_symbols_rgba_dev", "fri_hip_encode_image_rgba_symbols", "fri_hip_decode_image_rgba",
    "fri_hip_plan_owned_pixels", "fri_hip_tile_shape", "fri_hip_plan_tiled_create", "fri_hip_plan_tiled_destroy", "fri_hip_plan_tiled_tile", "fri_hip_plan_tiled_grid",
    "fri_hip_split_tiles_dev", "fri_hip_merge_tiles_dev", "fri_hip_encode_symbols_tiled_dev", "fri_hip_encode_image_tiled_symbols", "fri_hip_decode_image_tiled",
    "fri_hip_measure_distortion_tiled_dev", "fri_hip_estimate_size_tiled_dev", "fri_hip_estimate_size_tiled", "fri_hip_search_quality_tiled", "fri_hip_search_quality_tiled_dev",
    "fri_hip_search_quality_ssim_tiled", "fri_hip_search_quality_ssim_tiled_dev", "fri_hip_search_quality_for_size_tiled", "fri_hip_search_quality_for_size_tiled_dev",
    "fri_hip_rans_scratch_bytes", "fri_hip_rans_encode_planes_dev", "fri_hip_rans_time_planes_dev", "fri_hip_encode_image_tiled_coded",
    "fri_hip_plan_tiled_region", "fri_hip_merge_tiles_region_dev", "fri_hip_decode_region_tiled_dev", "fri_hip_decode_region_tiled",
    "fri_hip_plan_tiled_region_cover", "fri_hip_split_tiles_region_dev", "fri_hip_encode_symbols_region_tiled_dev", "fri_hip_encode_region_tiled_symbols",
    "fri_hip_tile_shape420", "fri_hip_plan_tiled420_create", "fri_hip_plan_tiled420_destroy", "fri_hip_plan_tiled420_luma", "fri_hip_plan_tiled420_chroma",
    "fri_hip_plan_tiled420_grid", "fri_hip_plan_tiled420_region", "fri_hip_plan_tiled420_buffer_tiles", "fri_hip_split_tiles420_dev", "fri_hip_merge_tiles420_dev",
    "fri_hip_merge_tiles420_region_dev", "fri_hip_encode_symbols_tiled420_dev", "fri_hip_encode_image_tiled420_symbols", "fri_hip_decode_image_tiled420",
    "fri_hip_decode_region_tiled420_dev", "fri_hip_decode_region_tiled420",
    "fri_hip_measure_distortion_tiled420_dev", "fri_hip_estimate_size_tiled420_dev", "fri_hip_estimate_size_tiled420", "fri_hip_search_quality_tiled420",
    "fri_hip_search_quality_tiled420_dev", "fri_hip_search_quality_ssim_tiled420", "fri_hip_search_quality_ssim_tiled420_dev", "fri_hip_search_quality_for_size_tiled420",
    "fri_hip_search_quality_for_size_tiled420_dev", "fri_hip_encode_image_tiled420_coded",
    "fri_hip_decode_scratch_bytes", "fri_hip_decode_planes_dev", "fri_hip_decode_time_planes_dev", "fri_hip_decode_image_tiled_coded", "fri_hip_decode_image_tiled420_coded",
    "fri_hip_plan_num_some_levels", "fri_hip_preview_size", "fri_hip_decode_planes_levels_dev", "fri_hip_preview_tiles_dev", "fri_hip_preview_image_tiled",
    "fri_hip_preview_image_tiled_coded",
    "fri_hip_plan_tiled_regions", "fri_hip_merge_tiles_regions_dev", "fri_hip_decode_regions_tiled_dev", "fri_hip_decode_regions_tiled",
    "fri_hip_decode_regions_tiled_coded",
    "fri_hip_plan_tiled420_regions", "fri_hip_merge_tiles420_regions_dev", "fri_hip_decode_regions_tiled420_dev", "fri_hip_decode_regions_tiled420",
    "fri_hip_decode_regions_tiled420_coded",
    "fri_hip_plan_tiled_preview_regions", "fri_hip_preview_tiles_regions_dev", "fri_hip_preview_regions_tiled", "fri_hip_preview_regions_tiled_coded",
    "fri_hip_plan_tiled_rgba_create", "fri_hip_plan_tiled_rgba_destroy", "fri_hip_plan_tiled_rgba_colour", "fri_hip_plan_tiled_rgba_alpha", "fri_hip_plan_tiled_rgba_grid",
    "fri_hip_plan_tiled_rgba_region", "fri_hip_plan_tiled_rgba_buffer_tiles", "fri_hip_split_tiles_rgba_dev", "fri_hip_merge_tiles_rgba_dev",
    "fri_hip_merge_tiles_rgba_region_dev", "fri_hip_encode_symbols_tiled_rgba_dev", "fri_hip_encode_image_tiled_rgba_symbols", "fri_hip_decode_image_tiled_rgba",
    "fri_hip_decode_region_tiled_rgba_dev", "fri_hip_decode_region_tiled_rgba",
]
DECODE_TRUNCATED, DECODE_BAD_MODEL, DECODE_BAD_SLOT = 1, 2, 4  # FRI_HIP_DECODE_*: bits of a plane's status word of fri_hip_decode_planes_dev (include/fri_hip.h)
RANS_EMPTY_OK = 1  # FRI_HIP_RANS_EMPTY_OK: `flags` of fri_hip_rans_encode_planes_dev - a context without counts is coded (the emitter's FRI_EMIT_EMPTY_OK)
RANS_TOO_SMALL, RANS_BAD_MODEL, RANS_ZERO_FREQ, RANS_BAD_BUCKET = 1, 2, 4, 8  # bits of a plane's status word (include/fri_hip.h)
TILED_ALLOW_HOLES = 1  # FRI_HIP_TILED_ALLOW_HOLES: `flags` of fri_hip_plan_tiled_create - accept a tile shape whose lattice does not own every pixel
ALPHA_KEEP, ALPHA_CLEAN = 0, 1  # `clean` of fri_hip_split_rgba_dev and the RGBA encodes: CLEAN zeroes the colour of pixels with A == 0
COLOUR_NONE, COLOUR_RCT, COLOUR_YCBCR = 0, 1, 3  # fri_hip_plan_set_colour_transform (bit 0: chroma planes, bit 1: irreversible)
DEQUANT_REFERENCE, DEQUANT_MULTIPLY, DEQUANT_MIDPOINT = 0, 1, 2  # fri_hip_plan_set_dequantiser


class FriHipError(RuntimeError):
    def __init__(self, code, where, detail=""):
        self.code = code
        msg = load_library().fri_hip_strerror(code).decode()
        super().__init__(f"{where}: {msg} ({code}){': ' + detail if detail else ''}")


def library_path():
    return _SO


def build_library(force=False):
    """Compile frave_amd/libfri_hip.so for gfx950 with hipcc (works without a GPU)."""
    src_dir = os.path.join(_HERE, "csrc")
    if force and os.path.exists(_SO):
        os.remove(_SO)
    subprocess.check_call(["make", "-s", "-C", src_dir])
    return _SO


_lib = None


def load_library():
    """Load libfri_hip.so. Raises if it has not been built -- there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise FileNotFoundError(f"{_SO} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). "
                                "frave_amd has no CPU fallback.")
    # One HIP runtime per process: torch bundles its own libamdhip64.so.7 (same SONAME as /opt/rocm's). If this
    # library were loaded first the dynamic linker would bind torch to /opt/rocm's copy later and torch then finds no
    # GPU; importing torch first makes both share torch's copy. Without torch (C++ callers) /opt/rocm's is used.
    if os.environ.get("FRI_HIP_NO_TORCH_PRELOAD") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(_SO)
    if os.environ.get("FRI_HIP_LIBRARY"):
        # an alternative build selected for an A/B measurement (tools/ab_lib.py) may predate the newest entry points: give those a stub that raises
        # when called, so that the older build still loads. The in-tree library gets no such leniency (tests/test_abi_symbols.py).
        def _missing(name):
            def stub(*a):
                raise AttributeError(f"{_SO} does not export {name}")
            return stub
        for name in SYMBOLS:
            try:
                getattr(L, name)
            except AttributeError:
                setattr(L, name, _missing(name))
    vp, u32, i32, sz = C.c_void_p, C.c_uint32, C.c_int, C.c_size_t
    L.fri_hip_strerror.restype = C.c_char_p
    L.fri_hip_strerror.argtypes = [i32]
    L.fri_hip_version.restype = C.c_char_p
    L.fri_hip_ctx_create.argtypes = [i32, C.POINTER(vp)]
    L.fri_hip_ctx_destroy.argtypes = [vp]
    L.fri_hip_backend.restype = C.c_char_p
    L.fri_hip_backend.argtypes = [vp]
    L.fri_hip_last_hip_error.restype = C.c_char_p
    L.fri_hip_last_hip_error.argtypes = [vp]
    L.fri_hip_plan_create.argtypes = [vp, u32, u32, u32, C.POINTER(vp)]
    L.fri_hip_plan_destroy.argtypes = [vp]
    for n in ("num_cells", "num_bfs_cells", "num_interior_cells"):
        f = getattr(L, "fri_hip_plan_" + n)
        f.restype, f.argtypes = u32, [vp]
    for n in ("coef_count", "pixel_bytes"):
        f = getattr(L, "fri_hip_plan_" + n)
        f.restype, f.argtypes = sz, [vp]
    L.fri_hip_plan_num_some.restype = C.c_uint64
    L.fri_hip_plan_num_some.argtypes = [vp]
    for n in ("centers", "valid_mask", "neighbour_cells", "neighbour_table", "tiling"):
        getattr(L, "fri_hip_plan_" + n).argtypes = [vp, vp]
    L.fri_hip_plan_tile_table.argtypes = [vp, vp, vp, vp]
    L.fri_hip_transform_quant.argtypes = [vp, vp, vp, vp]
    L.fri_hip_transform_quant_dev.argtypes = [vp, vp, vp, vp, vp]
    L.fri_hip_transform_quant_batch_dev.argtypes = [vp, u32, vp, sz, vp, vp, sz, vp]
    L.fri_hip_transform_quant_batch.argtypes = [vp, u32, vp, vp, vp]
    L.fri_hip_predict_histogram.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp, vp]
    L.fri_hip_predict_histogram_dev.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp, vp, vp]
    L.fri_hip_fit_value_sums.argtypes = [vp, vp, u32, vp]
    L.fri_hip_fit_value_sums_dev.argtypes = [vp, vp, u32, vp, vp]
    L.fri_hip_fit_width_sums.argtypes = [vp, vp, u32, vp, vp, vp, vp]
    L.fri_hip_fit_width_sums_dev.argtypes = [vp, vp, u32, vp, vp, vp, vp]
    L.fri_hip_inverse_transform.argtypes = [vp, vp, vp, vp]
    L.fri_hip_inverse_transform_dev.argtypes = [vp, vp, vp, vp, vp]
    L.fri_hip_plan_read_trace.argtypes = [vp, vp]
    L.fri_hip_plan_inverse_lists.argtypes = [vp, vp]
    L.fri_hip_plan_predict_grid.argtypes = [vp, vp]
    L.fri_hip_plan_pred_slots.argtypes = [vp, vp]
    L.fri_hip_time_transform_quant_dev.argtypes = [vp, u32, vp, sz, vp, vp, sz, u32, vp, C.POINTER(C.c_double)]
    L.fri_hip_time_transform_quant_streams_dev.argtypes = [vp, u32, vp, sz, vp, vp, sz, u32, u32, C.POINTER(C.c_double)]
    L.fri_hip_plan_tune_forward.argtypes = [vp, u32, C.c_char_p, sz]
    L.fri_hip_shard_size.restype, L.fri_hip_shard_size.argtypes = u32, [u32, u32, u32]
    L.fri_hip_shard_image.restype, L.fri_hip_shard_image.argtypes = u32, [u32, u32, u32]
    L.fri_hip_multi_create.argtypes = [vp, u32, u32, u32, u32, C.POINTER(vp)]
    L.fri_hip_multi_destroy.argtypes = [vp]
    L.fri_hip_multi_num_devices.restype, L.fri_hip_multi_num_devices.argtypes = u32, [vp]
    L.fri_hip_multi_plan.restype, L.fri_hip_multi_plan.argtypes = vp, [vp, u32]
    L.fri_hip_multi_transform_quant.argtypes = [vp, u32, vp, vp, vp]
    L.fri_hip_predict_histogram_batch_dev.argtypes = [vp, u32, vp, sz, vp, vp, vp, sz, vp, vp, vp]
    L.fri_hip_fit_value_sums_batch_dev.argtypes = [vp, u32, vp, sz, vp, vp]
    L.fri_hip_fit_width_sums_batch_dev.argtypes = [vp, u32, vp, sz, vp, vp, vp, vp]
    L.fri_hip_solve6.restype, L.fri_hip_solve6.argtypes = None, [vp, vp, vp]
    L.fri_hip_fit_value_params.restype, L.fri_hip_fit_value_params.argtypes = None, [vp, vp]
    L.fri_hip_fit_width_params.restype, L.fri_hip_fit_width_params.argtypes = None, [vp, vp, vp, vp]
    L.fri_hip_encode_image.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.fri_hip_encode_image_dev.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.fri_hip_inverse_transform_batch_dev.argtypes = [vp, u32, vp, sz, vp, vp, sz, vp]
    L.fri_hip_predict_image.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.fri_hip_predict_image_dev.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.fri_hip_fit_params_batch_dev.argtypes = [vp, u32, vp, sz, vp, vp, vp]
    L.fri_hip_plan_assume_forward_coefficients.argtypes = [vp, i32]
    L.fri_hip_plan_set_dequantiser.argtypes = [vp, i32]
    L.fri_hip_plan_set_colour_transform.argtypes = [vp, i32]
    L.fri_hip_quality_matrix.argtypes = [i32, vp]
    L.fri_hip_measure_distortion_dev.argtypes = [vp, vp, vp, vp, vp, vp]
    L.fri_hip_search_quality.argtypes = [vp, vp, C.c_double, vp, vp]
    L.fri_hip_search_quality_dev.argtypes = [vp, vp, C.c_double, vp, vp, vp]
    L.fri_hip_estimate_size_dev.argtypes = [vp, u32, vp, vp, vp, vp, vp]
    L.fri_hip_estimate_size.argtypes = [vp, vp, vp, vp]
    L.fri_hip_search_quality_for_size.argtypes = [vp, vp, C.c_uint64, vp, vp]
    L.fri_hip_search_quality_for_size_dev.argtypes = [vp, vp, C.c_uint64, vp, vp, vp]
    L.fri_hip_measure_ssim_dev.argtypes = [vp, u32, vp, vp, sz, vp, vp]
    L.fri_hip_measure_ssim.argtypes = [vp, vp, vp, vp]
    L.fri_hip_search_quality_ssim.argtypes = [vp, vp, C.c_double, vp, vp]
    L.fri_hip_search_quality_ssim_dev.argtypes = [vp, vp, C.c_double, vp, vp, vp]
    L.fri_hip_plan_set_stream_order.argtypes = [vp, vp, C.c_uint64]
    L.fri_hip_symbol_stream_batch_dev.argtypes = [vp, u32, vp, sz, vp, vp, sz, vp, sz, vp]
    L.fri_hip_encode_image_symbols.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp]
    L.fri_hip_encode_symbols_batch_dev.argtypes = [vp, u32, vp, sz, vp, i32, vp, vp, sz, vp, sz, vp, sz, vp, vp, vp, vp]
    L.fri_hip_encode_image_batch.argtypes = [vp, u32, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.fri_hip_multi_encode_image.argtypes = [vp, u32, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.fri_hip_fit_value_params_batch_dev.argtypes = [vp, u32, vp, vp, vp]
    L.fri_hip_fit_width_params_batch_dev.argtypes = [vp, u32, vp, vp, vp, vp]
    L.fri_hip_encode_image_batch_dev.argtypes = [vp, u32, vp, sz, vp, i32, vp, vp, sz, vp, vp, sz, vp, vp, vp, vp]
    L.fri_hip_plan420_create.argtypes = [vp, u32, u32, C.POINTER(vp)]
    L.fri_hip_plan420_destroy.argtypes = [vp]
    L.fri_hip_plan420_luma.restype, L.fri_hip_plan420_luma.argtypes = vp, [vp]
    L.fri_hip_plan420_chroma.restype, L.fri_hip_plan420_chroma.argtypes = vp, [vp]
    L.fri_hip_split420_dev.argtypes = [vp, vp, vp, vp, vp]
    L.fri_hip_merge420_dev.argtypes = [vp, vp, vp, vp, vp]
    L.fri_hip_measure_distortion420_dev.argtypes = [vp, vp, vp, vp, vp, vp]
    L.fri_hip_encode_image420_symbols.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
    L.fri_hip_decode_image420.argtypes = [vp, vp, i32, vp]
    L.fri_hip_search_quality420.argtypes = [vp, vp, C.c_double, vp, vp]
    L.fri_hip_search_quality420_dev.argtypes = [vp, vp, C.c_double, vp, vp, vp]
    L.fri_hip_search_quality_for_size420.argtypes = [vp, vp, C.c_uint64, vp, vp]
    L.fri_hip_search_quality_for_size420_dev.argtypes = [vp, vp, C.c_uint64, vp, vp, vp]
    L.fri_hip_search_quality_ssim420.argtypes = [vp, vp, C.c_double, vp, vp]
    L.fri_hip_search_quality_ssim420_dev.argtypes = [vp, vp, C.c_double, vp, vp, vp]
    L.fri_hip_plan_rgba_create.argtypes = [vp, u32, u32, C.POINTER(vp)]
    L.fri_hip_plan_rgba_destroy.argtypes = [vp]
    L.fri_hip_plan_rgba_colour.restype, L.fri_hip_plan_rgba_colour.argtypes = vp, [vp]
    L.fri_hip_plan_rgba_alpha.restype, L.fri_hip_plan_rgba_alpha.argtypes = vp, [vp]
    L.fri_hip_split_rgba_dev.argtypes = [vp, vp, i32, vp, vp, vp]
    L.fri_hip_merge_rgba_dev.argtypes = [vp, vp, vp, vp, vp]
    L.fri_hip_encode_symbols_rgba_dev.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp]
    L.fri_hip_encode_image_rgba_symbols.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.fri_hip_decode_image_rgba.argtypes = [vp, vp, vp, vp]
    L.fri_hip_plan_owned_pixels.restype, L.fri_hip_plan_owned_pixels.argtypes = C.c_uint64, [vp]
    L.fri_hip_tile_shape.argtypes = [u32, u32, u32, vp, vp]
    L.fri_hip_plan_tiled_create.argtypes = [vp, u32, u32, u32, u32, u32, u32, C.POINTER(vp)]
    L.fri_hip_plan_tiled_destroy.argtypes = [vp]
    L.fri_hip_plan_tiled_tile.restype, L.fri_hip_plan_tiled_tile.argtypes = vp, [vp]
    L.fri_hip_plan_tiled_grid.argtypes = [vp, vp]
    L.fri_hip_split_tiles_dev.argtypes = [vp, vp, vp, vp]
    L.fri_hip_merge_tiles_dev.argtypes = [vp, vp, vp, vp]
    L.fri_hip_encode_symbols_tiled_dev.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.fri_hip_encode_image_tiled_symbols.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.fri_hip_decode_image_tiled.argtypes = [vp, vp, vp, vp]
    L.fri_hip_plan_tiled_region.argtypes = [vp, u32, u32, u32, u32, vp]
    L.fri_hip_merge_tiles_region_dev.argtypes = [vp, vp, u32, u32, u32, u32, vp, vp]
    L.fri_hip_decode_region_tiled_dev.argtypes = [vp, vp, vp, u32, u32, u32, u32, vp, vp]
    L.fri_hip_decode_region_tiled.argtypes = [vp, vp, vp, u32, u32, u32, u32, vp]
    L.fri_hip_plan_tiled_regions.argtypes = [vp, u32, vp, vp, C.c_size_t, vp, vp, C.c_size_t]
    L.fri_hip_merge_tiles_regions_dev.argtypes = [vp, vp, u32, u32, vp, vp, vp]
    L.fri_hip_decode_regions_tiled_dev.argtypes = [vp, vp, vp, u32, vp, vp, vp]
    L.fri_hip_decode_regions_tiled.argtypes = [vp, vp, vp, u32, vp, vp]
    L.fri_hip_decode_regions_tiled_coded.argtypes = [vp, u32, vp, vp, C.c_size_t, vp, vp, vp, vp, vp, vp, vp, vp]
    L.fri_hip_plan_tiled_region_cover.argtypes = [vp, u32, u32, u32, u32, vp]
    L.fri_hip_split_tiles_region_dev.argtypes = [vp, vp, C.c_size_t, u32, u32, u32, u32, u32, u32, u32, u32, vp, vp]
    L.fri_hip_encode_symbols_region_tiled_dev.argtypes = [vp, vp, C.c_size_t, u32, u32, u32, u32, u32, u32, u32, u32, vp, i32, vp, vp, vp, vp, vp, vp]
    L.fri_hip_encode_region_tiled_symbols.argtypes = [vp, vp, u32, u32, u32, u32, vp, vp, vp, vp, vp, vp]
    L.fri_hip_measure_distortion_tiled_dev.argtypes = [vp, vp, vp, vp, vp]
    L.fri_hip_estimate_size_tiled_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.fri_hip_estimate_size_tiled.argtypes = [vp, vp, vp, vp, vp]
    L.fri_hip_rans_scratch_bytes.restype, L.fri_hip_rans_scratch_bytes.argtypes = C.c_uint64, [u32, C.c_uint64]
    L.fri_hip_rans_encode_planes_dev.argtypes = [vp, u32, vp, sz, C.c_uint64, vp, u32, vp, sz, vp, vp, vp, vp, vp, vp]
    L.fri_hip_rans_time_planes_dev.argtypes = [vp, u32, vp, sz, C.c_uint64, vp, u32, vp, sz, vp, vp, vp, vp, vp, vp, vp]
    L.fri_hip_encode_image_tiled_coded.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp]
    L.fri_hip_search_quality_tiled.argtypes = [vp, vp, C.c_double, vp, vp]
    L.fri_hip_search_quality_tiled_dev.argtypes = [vp, vp, C.c_double, vp, vp, vp]
    L.fri_hip_search_quality_ssim_tiled.argtypes = [vp, vp, C.c_double, vp, vp]
    L.fri_hip_search_quality_ssim_tiled_dev.argtypes = [vp, vp, C.c_double, vp, vp, vp]
    L.fri_hip_search_quality_for_size_tiled.argtypes = [vp, vp, C.c_uint64, vp, vp]
    L.fri_hip_search_quality_for_size_tiled_dev.argtypes = [vp, vp, C.c_uint64, vp, vp, vp]
    L.fri_hip_tile_shape420.argtypes = [u32, u32, u32, vp, vp]
    L.fri_hip_plan_tiled420_create.argtypes = [vp, u32, u32, u32, u32, u32, C.POINTER(vp)]
    L.fri_hip_plan_tiled420_destroy.argtypes = [vp]
    L.fri_hip_plan_tiled420_luma.restype, L.fri_hip_plan_tiled420_luma.argtypes = vp, [vp]
    L.fri_hip_plan_tiled420_chroma.restype, L.fri_hip_plan_tiled420_chroma.argtypes = vp, [vp]
    L.fri_hip_plan_tiled420_grid.argtypes = [vp, vp]
    L.fri_hip_plan_tiled420_region.argtypes = [vp, u32, u32, u32, u32, vp]
    L.fri_hip_plan_tiled420_buffer_tiles.argtypes = [vp, vp]
    L.fri_hip_split_tiles420_dev.argtypes = [vp, vp, vp, vp, vp]
    L.fri_hip_merge_tiles420_dev.argtypes = [vp, vp, vp, vp, vp]
    L.fri_hip_merge_tiles420_region_dev.argtypes = [vp, vp, vp, u32, u32, u32, u32, vp, vp]
    L.fri_hip_encode_symbols_tiled420_dev.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.fri_hip_encode_image_tiled420_symbols.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
    L.fri_hip_decode_image_tiled420.argtypes = [vp, vp, i32, vp]
    L.fri_hip_decode_region_tiled420_dev.argtypes = [vp, vp, i32, u32, u32, u32, u32, vp, vp]
    L.fri_hip_decode_region_tiled420.argtypes = [vp, vp, i32, u32, u32, u32, u32, vp]
    L.fri_hip_plan_tiled420_regions.argtypes = [vp, u32, vp, vp, C.c_size_t, vp, vp, C.c_size_t]
    L.fri_hip_merge_tiles420_regions_dev.argtypes = [vp, vp, vp, u32, u32, vp, vp, vp]
    L.fri_hip_decode_regions_tiled420_dev.argtypes = [vp, vp, i32, u32, vp, vp, vp]
    L.fri_hip_decode_regions_tiled420.argtypes = [vp, vp, i32, u32, vp, vp]
    L.fri_hip_decode_regions_tiled420_coded.argtypes = [vp, u32, vp, vp, C.c_size_t, vp, vp, vp, vp, vp, i32, vp, vp]
    L.fri_hip_measure_distortion_tiled420_dev.argtypes = [vp, vp, vp, vp, vp, vp]
    L.fri_hip_estimate_size_tiled420_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.fri_hip_estimate_size_tiled420.argtypes = [vp, vp, vp, vp, vp]
    L.fri_hip_search_quality_tiled420.argtypes = [vp, vp, C.c_double, vp, vp]
    L.fri_hip_search_quality_tiled420_dev.argtypes = [vp, vp, C.c_double, vp, vp, vp]
    L.fri_hip_search_quality_ssim_tiled420.argtypes = [vp, vp, C.c_double, vp, vp]
    L.fri_hip_search_quality_ssim_tiled420_dev.argtypes = [vp, vp, C.c_double, vp, vp, vp]
    L.fri_hip_search_quality_for_size_tiled420.argtypes = [vp, vp, C.c_uint64, vp, vp]
    L.fri_hip_search_quality_for_size_tiled420_dev.argtypes = [vp, vp, C.c_uint64, vp, vp, vp]
    L.fri_hip_plan_tiled_rgba_create.argtypes = [vp, u32, u32, u32, u32, u32, C.POINTER(vp)]
    L.fri_hip_plan_tiled_rgba_destroy.argtypes = [vp]
    L.fri_hip_plan_tiled_rgba_colour.restype, L.fri_hip_plan_tiled_rgba_colour.argtypes = vp, [vp]
    L.fri_hip_plan_tiled_rgba_alpha.restype, L.fri_hip_plan_tiled_rgba_alpha.argtypes = vp, [vp]
    L.fri_hip_plan_tiled_rgba_grid.argtypes = [vp, vp]
    L.fri_hip_plan_tiled_rgba_region.argtypes = [vp, u32, u32, u32, u32, vp]
    L.fri_hip_plan_tiled_rgba_buffer_tiles.argtypes = [vp, vp]
    L.fri_hip_split_tiles_rgba_dev.argtypes = [vp, vp, i32, vp, vp, vp]
    L.fri_hip_merge_tiles_rgba_dev.argtypes = [vp, vp, vp, vp, vp]
    L.fri_hip_merge_tiles_rgba_region_dev.argtypes = [vp, vp, vp, u32, u32, u32, u32, vp, vp]
    L.fri_hip_encode_symbols_tiled_rgba_dev.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp]
    L.fri_hip_encode_image_tiled_rgba_symbols.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.fri_hip_decode_image_tiled_rgba.argtypes = [vp, vp, vp, vp]
    L.fri_hip_decode_region_tiled_rgba_dev.argtypes = [vp, vp, vp, u32, u32, u32, u32, vp, vp]
    L.fri_hip_decode_region_tiled_rgba.argtypes = [vp, vp, vp, u32, u32, u32, u32, vp]
    L.fri_hip_encode_image_tiled420_coded.argtypes = [vp, vp, i32, vp, vp, vp, sz, vp, vp, vp, vp]
    L.fri_hip_decode_scratch_bytes.restype, L.fri_hip_decode_scratch_bytes.argtypes = C.c_uint64, [u32]
    L.fri_hip_decode_planes_dev.argtypes = [vp, u32, vp, sz, vp, vp, vp, vp, vp, vp, sz, vp, vp, vp]
    L.fri_hip_decode_time_planes_dev.argtypes = [vp, u32, vp, sz, vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp]
    L.fri_hip_decode_image_tiled_coded.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp]
    L.fri_hip_decode_image_tiled420_coded.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, i32, vp, vp]
    L.fri_hip_plan_num_some_levels.argtypes = [vp, u32, vp]
    L.fri_hip_preview_size.argtypes = [u32, u32, u32, vp]
    L.fri_hip_decode_planes_levels_dev.argtypes = [vp, u32, vp, sz, vp, vp, vp, vp, vp, vp, sz, u32, vp, vp, vp]
    L.fri_hip_preview_tiles_dev.argtypes = [vp, vp, sz, u32, u32, u32, vp, vp, vp]
    L.fri_hip_preview_image_tiled.argtypes = [vp, vp, u32, u32, vp, vp]
    L.fri_hip_preview_image_tiled_coded.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, u32, u32, vp, vp, vp]
    L.fri_hip_plan_tiled_preview_regions.argtypes = [vp, u32, u32, vp, vp, sz, vp, vp, sz]
    L.fri_hip_preview_tiles_regions_dev.argtypes = [vp, vp, sz, u32, u32, u32, vp, u32, u32, vp, vp, vp]
    L.fri_hip_preview_regions_tiled.argtypes = [vp, vp, u32, u32, vp, u32, vp, vp]
    L.fri_hip_preview_regions_tiled_coded.argtypes = [vp, u32, vp, vp, sz, vp, vp, vp, vp, vp, u32, u32, vp, vp, vp]
    _lib = L
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _q(q):
    q = np.ones(32, np.int32) if q is None else np.ascontiguousarray(q, np.int32)
    assert q.size == 32
    return q


def _untriangle(tri, n):
    """[g][n(n+1)/2] upper triangle (row major) -> [g][n][n] symmetric."""
    out = np.zeros((tri.shape[0], n, n), tri.dtype)
    iu = np.triu_indices(n)
    for g in range(tri.shape[0]):
        out[g][iu] = tri[g]
        out[g] = out[g] + out[g].T - np.diag(np.diag(out[g]))
    return out


def solve_normal_equations(ata, atb, eps=1e-12):
    """Minimum-norm least-squares solution from normal equations (what lstsq's SVD returns, up to rounding):
    x = pinv(A^T A) A^T b via the symmetric eigen-decomposition; eigenvalues <= eps * max are treated as zero."""
    ata = np.asarray(ata, np.float64)
    atb = np.asarray(atb, np.float64)
    lam, vec = np.linalg.eigh(ata)
    keep = lam > eps * max(lam.max(), 0.0)
    inv = np.where(keep, 1.0 / np.where(keep, lam, 1.0), 0.0)
    return (vec * inv) @ (vec.T @ atb)


def _check(rc, where, ctx=None):
    if rc != 0:
        detail = ""
        if ctx is not None and ctx._h:
            detail = load_library().fri_hip_last_hip_error(ctx._h).decode()
        raise FriHipError(rc, where, detail)


def shard_images(n_images, shard, n_shards):
    """Global indices of the images of `shard` (fri_hip_shard_size / fri_hip_shard_image: image i -> shard i mod n_shards)."""
    L = load_library()
    return [L.fri_hip_shard_image(k, shard, n_shards) for k in range(L.fri_hip_shard_size(n_images, shard, n_shards))]


def tile_shape(width, height, target=512):
    """fri_hip_tile_shape: (tile_w, tile_h) of about target x target for a width x height image - the first shape of the documented walk whose C = 1 lattice owns
    every pixel; FriHipError with code -7 when the walk finds none. Host only."""
    tw, th = C.c_uint32(0), C.c_uint32(0)
    _check(load_library().fri_hip_tile_shape(width, height, target, C.addressof(tw), C.addressof(th)), "fri_hip_tile_shape")
    return tw.value, th.value


def tile_shape420(width, height, target=512):
    """fri_hip_tile_shape420: (tile_w, tile_h) of about target x target for tiled 4:2:0 coding - the first shape of tile_shape's walk at which the C = 1 lattice of
    the tile AND the C = 1 lattice of its (tile_w + 1) / 2 x (tile_h + 1) / 2 chroma planes own every pixel; FriHipError with code -7 when the walk finds none.
    Host only."""
    tw, th = C.c_uint32(0), C.c_uint32(0)
    _check(load_library().fri_hip_tile_shape420(width, height, target, C.addressof(tw), C.addressof(th)), "fri_hip_tile_shape420")
    return tw.value, th.value


def rans_scratch_bytes(n_planes, n_symbols):
    """fri_hip_rans_scratch_bytes: the device scratch fri_hip_rans_encode_planes_dev needs for n_planes planes of n_symbols symbols (0: counts out of range)."""
    return int(load_library().fri_hip_rans_scratch_bytes(n_planes, n_symbols))


def rans_encode_planes_dev(ctx, n_planes, d_symbols, symbol_stride, n_symbols, d_hist, flags, d_words, word_stride, d_n_words, d_models, d_off_values, d_status, d_scratch,
                           stream=0, timed=False):
    """fri_hip_rans_encode_planes_dev (K11), device pointers as ints: d_symbols uint16 streams symbol_stride apart, d_hist uint32 [n_planes][10][1024] -> d_words uint32
    [n_planes][word_stride], d_n_words uint32 [n_planes], d_models uint32 [n_planes][10][4], d_off_values uint16 [n_planes][10][1024], d_status uint32 [n_planes][4];
    d_scratch: rans_scratch_bytes(..) bytes, 256-byte aligned. Only enqueues. timed=True: fri_hip_rans_time_planes_dev - synchronises and returns the microseconds of
    the model, coder and stitch kernels."""
    L = load_library()
    args = (ctx._h if ctx else None, n_planes, d_symbols, symbol_stride, n_symbols, d_hist, flags, d_words, word_stride, d_n_words, d_models, d_off_values, d_status, d_scratch,
            stream)
    if timed:
        us = np.zeros(3, np.float64)
        _check(L.fri_hip_rans_time_planes_dev(*args, _p(us)), "fri_hip_rans_time_planes_dev", ctx)
        return us
    _check(L.fri_hip_rans_encode_planes_dev(*args), "fri_hip_rans_encode_planes_dev", ctx)


def decode_scratch_bytes(n_planes):
    """fri_hip_decode_scratch_bytes: the device scratch fri_hip_decode_planes_dev needs for n_planes planes (0: count out of range)."""
    return int(load_library().fri_hip_decode_scratch_bytes(n_planes))


def decode_planes_dev(plan, n_planes, d_words, word_stride, d_n_words, d_models, d_off_values, d_value_params, d_width_params, d_coefs, coef_stride, d_status, d_scratch,
                      stream=0, timed=False, levels=None):
    """fri_hip_decode_planes_dev (K13), device pointers as ints: the coded planes of emit.tiled_parse_coded - d_words uint32 [n_planes][word_stride], d_n_words
    [n_planes], d_models [n_planes][10][4], d_off_values uint16 [n_planes][10][1024], d_value_params / d_width_params f32 [n_planes][3][6] - on the lattice of `plan`
    (which needs its stream order) -> d_coefs int32, plane p at + p * coef_stride elements, and d_status uint32 [n_planes][4] = {bits, at, 0, 0}. d_scratch:
    decode_scratch_bytes(..) bytes, 256-byte aligned. Only enqueues. timed=True: fri_hip_decode_time_planes_dev - synchronises and returns the microseconds of the
    model and decode kernels. levels (0..9): fri_hip_decode_planes_levels_dev - the step loop stops behind the nodes with heap index < 2^levels."""
    L = load_library()
    args = (plan._h if plan else None, n_planes, d_words, word_stride, d_n_words, d_models, d_off_values, d_value_params, d_width_params, d_coefs, coef_stride, d_status,
            d_scratch, stream)
    ctx = plan.ctx if plan else None
    if levels is not None:
        assert not timed
        _check(L.fri_hip_decode_planes_levels_dev(*args[:11], int(levels), *args[11:]), "fri_hip_decode_planes_levels_dev", ctx)
        return
    if timed:
        us = np.zeros(2, np.float64)
        _check(L.fri_hip_decode_time_planes_dev(*args, _p(us)), "fri_hip_decode_time_planes_dev", ctx)
        return us
    _check(L.fri_hip_decode_planes_dev(*args), "fri_hip_decode_planes_dev", ctx)


def preview_size(width, height, shift):
    """fri_hip_preview_size: (w', h') = (ceil(W / 2^shift), ceil(H / 2^shift)) of a thumbnail, shift 0..4. Needs no GPU."""
    out = np.zeros(2, np.uint32)
    _check(load_library().fri_hip_preview_size(width, height, shift, _p(out)), "fri_hip_preview_size")
    return int(out[0]), int(out[1])


def _coded_planes(coded, planes):
    """the arrays of emit.tiled_parse_coded (with or without its leading TiledInfo) as the C ABI takes them"""
    words, n_words, models, off, vp, wp = coded[-6:]
    words, n_words, models = np.ascontiguousarray(words, np.uint32), np.ascontiguousarray(n_words, np.uint32), np.ascontiguousarray(models, np.uint32)
    off, vp, wp = np.ascontiguousarray(off, np.uint16), np.ascontiguousarray(vp, np.float32), np.ascontiguousarray(wp, np.float32)
    assert n_words.size == planes and words.ndim == 2 and words.shape[0] == planes and models.size == planes * 40 and off.size == planes * 10240
    assert vp.size == planes * 18 and wp.size == planes * 18
    return words, n_words, models, off, vp, wp


def _check_decode(rc, where, ctx, status):
    """_check, with the planes' status on the error a refused plane raises (-1 with the status filled)"""
    try:
        _check(rc, where, ctx)
    except FriHipError as e:
        e.status = status
        raise


def quality_matrix(quality):
    """fri_hip_quality_matrix: the int32 [32] quantisation matrix of quality 1..100 (100 = all ones, lossless). Needs no GPU."""
    out = np.empty(32, np.int32)
    _check(load_library().fri_hip_quality_matrix(int(quality), _p(out)), "fri_hip_quality_matrix")
    return out


def distortion_psnr(measure, channels):
    """PSNR in dB of a fri_hip_measure_distortion_dev result (uint64 [2 C + 1]): 10 log10(255^2 N / SSE) pooled over the channels,
    N = owned pixels x C; +inf when SSE = 0."""
    m = [int(x) for x in np.asarray(measure).ravel()[: 2 * channels + 1]]
    sse = sum(m[2 * c] for c in range(channels))
    if sse == 0:
        return float("inf")
    return 10.0 * np.log10(255.0 * 255.0 * m[2 * channels] * channels / sse)


def ssim_of(measure, channels):
    """(SSIM, [SSIM_c per channel]) of a fri_hip_measure_ssim result (int64 [C + 1]: the channels' sums of window values in units of 2^-32, then the
    window count N): SSIM = (sum over c of sum_c) / (C N 2^32), the integer sum first; SSIM_c = sum_c / (N 2^32)."""
    m = [int(x) for x in np.asarray(measure).ravel()[: channels + 1]]
    n = m[channels]
    return float(sum(m[:channels])) / (float(channels * n) * 2.0 ** 32), [float(m[c]) / (float(n) * 2.0 ** 32) for c in range(channels)]


def fit_value_params(gram_tri):
    """fri_hip_fit_value_params: gram_tri int64 [3][28] (upper triangles) -> float32 [3][6]."""
    g = np.ascontiguousarray(gram_tri, np.int64).reshape(3, 28)
    out = np.empty((3, 6), np.float32)
    load_library().fri_hip_fit_value_params(_p(g), _p(out))
    return out


def fit_width_params(wtw_tri, wtr, rows):
    """fri_hip_fit_width_params: wtw_tri int64 [3][21], wtr float64 [3][6], rows uint64 [3] -> float32 [3][6]."""
    w = np.ascontiguousarray(wtw_tri, np.int64).reshape(3, 21)
    r = np.ascontiguousarray(wtr, np.float64).reshape(3, 6)
    n = np.ascontiguousarray(rows, np.uint64).reshape(3)
    out = np.empty((3, 6), np.float32)
    load_library().fri_hip_fit_width_params(_p(w), _p(r), _p(n), _p(out))
    return out


def _search(plan, name, pixels, target, ctype, stream):
    """A quality search of any plan kind: entry point `name` (pixels: a host array) or `name`_dev (pixels: a device pointer, an int) -> (quality, the value there)."""
    qual, v = C.c_int32(0), ctype(0)
    L = load_library()
    if isinstance(pixels, int):
        _check(getattr(L, name + "_dev")(plan._h, pixels, target, C.byref(qual), C.byref(v), stream), name + "_dev", plan.ctx)
    else:
        px = np.ascontiguousarray(pixels, np.uint8)
        assert px.size == plan.pixel_bytes
        _check(getattr(L, name)(plan._h, _p(px), target, C.byref(qual), C.byref(v)), name, plan.ctx)
    return qual.value, v.value


def _encode_batch(fn, handle, where, ctx, images, channels, num_cells, qmatrix, fit, params, want_bucket, want_prediction):
    """Shared marshalling of fri_hip_encode_image_batch / fri_hip_multi_encode_image: lists of per-image arrays."""
    imgs = [np.ascontiguousarray(i, np.uint8).reshape(-1) for i in images]
    n, c, f = len(imgs), channels, num_cells
    if params is None:
        par = [np.zeros((c, 2, 3, 6), np.float32) for _ in imgs]
    else:
        par = [np.ascontiguousarray(p, np.float32).reshape(c, 2, 3, 6).copy() for p in params]
    coefs = [np.empty((c, f, 512), np.int32) for _ in imgs]
    bucket = [np.empty((c, f, 512), np.uint8) for _ in imgs] if want_bucket else None
    pred = [np.empty((c, f, 512), np.int32) for _ in imgs] if want_prediction else None
    hist = [np.empty((c, 10, 1024), np.uint32) for _ in imgs]
    oob = [np.zeros(c, np.uint64) for _ in imgs]
    arr = lambda xs: (C.c_void_p * n)(*[x.ctypes.data for x in xs]) if xs is not None else None
    q = _q(qmatrix)
    _check(fn(handle, n, arr(imgs), _p(q), 1 if fit else 0, arr(par), arr(coefs), arr(bucket), arr(pred), arr(hist), arr(oob)), where, ctx)
    return coefs, par, bucket, pred, hist, oob


class Multi:
    """fri_hip_multi: one process driving several GPUs, one ctx + plan per device, image i on devices[i mod len(devices)]."""

    def __init__(self, devices, width, height, channels):
        self._h = None
        h = C.c_void_p()
        dev = (C.c_int * len(devices))(*devices)
        _check(load_library().fri_hip_multi_create(dev, len(devices), width, height, channels, C.byref(h)), "fri_hip_multi_create")
        self._h = h
        self.channels = channels
        L = load_library()
        self.num_devices = L.fri_hip_multi_num_devices(h)
        self.num_cells = L.fri_hip_plan_num_cells(L.fri_hip_multi_plan(h, 0))

    def transform_quant(self, images, qmatrix=None):
        imgs = [np.ascontiguousarray(i, np.uint8).reshape(-1) for i in images]
        outs = [np.empty((self.channels, self.num_cells, 512), np.int32) for _ in imgs]
        n = len(imgs)
        pin = (C.c_void_p * n)(*[i.ctypes.data for i in imgs])
        pout = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        q = _q(qmatrix)
        _check(load_library().fri_hip_multi_transform_quant(self._h, n, pin, _p(q), pout), "fri_hip_multi_transform_quant")
        return outs

    def encode_image(self, images, qmatrix=None, fit=True, params=None, want_bucket=True, want_prediction=True):
        """fri_hip_multi_encode_image: per image (coefs, params [C][2][3][6], bucket, prediction, hist, oob), image i on device i mod N."""
        return _encode_batch(load_library().fri_hip_multi_encode_image, self._h, "fri_hip_multi_encode_image", None, images, self.channels, self.num_cells, qmatrix, fit, params,
                             want_bucket, want_prediction)

    def set_colour_transform(self, mode):
        """fri_hip_plan_set_colour_transform on every device's plan (see Plan.set_colour_transform)."""
        L = load_library()
        for d in range(self.num_devices):
            _check(L.fri_hip_plan_set_colour_transform(L.fri_hip_multi_plan(self._h, d), int(mode)), "fri_hip_plan_set_colour_transform")

    def close(self):
        if self._h:
            load_library().fri_hip_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """fri_hip_ctx: one per (host thread, GPU). Raises FriHipError(NO_DEVICE) without a gfx950 GPU."""

    def __init__(self, device=0):
        self._h = None
        h = C.c_void_p()
        _check(load_library().fri_hip_ctx_create(device, C.byref(h)), "fri_hip_ctx_create")
        self._h = h
        self.device = device

    @property
    def backend(self):
        return load_library().fri_hip_backend(self._h).decode()

    def close(self):
        if self._h:
            load_library().fri_hip_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Plan:
    """fri_hip_plan: geometry of one (width, height, channels). ctx=None gives a host-only plan (getters only)."""

    def __init__(self, ctx, width, height, channels, _handle=None):
        self._h = None
        self.ctx = ctx
        self.width, self.height, self.channels = width, height, channels
        self.colour_transform = COLOUR_NONE
        self._owns = _handle is None
        if _handle is None:
            h = C.c_void_p()
            _check(load_library().fri_hip_plan_create(ctx._h if ctx else None, width, height, channels, C.byref(h)), "fri_hip_plan_create", ctx)
        else:  # a view of a plan somebody else owns (Plan420's inner plans): close() leaves it alone
            h = C.c_void_p(_handle)
        self._h = h
        L = load_library()
        self.num_cells = L.fri_hip_plan_num_cells(h)
        self.num_bfs_cells = L.fri_hip_plan_num_bfs_cells(h)
        self.num_interior_cells = L.fri_hip_plan_num_interior_cells(h)
        self.coef_count = L.fri_hip_plan_coef_count(h)
        self.pixel_bytes = L.fri_hip_plan_pixel_bytes(h)
        self.num_some = L.fri_hip_plan_num_some(h)

    def close(self):
        if self._h:
            if self._owns:
                load_library().fri_hip_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def num_some_levels(self, levels):
        """fri_hip_plan_num_some_levels: the Some coefficients with heap index < 2^levels per channel (levels 0..9) - the length of the stream's prefix that holds
        them; num_some_levels(9) == num_some. Works on a host-only plan."""
        out = C.c_uint64(0)
        _check(load_library().fri_hip_plan_num_some_levels(self._h, int(levels), C.byref(out)), "fri_hip_plan_num_some_levels", self.ctx)
        return int(out.value)

    def owned_pixels(self):
        """fri_hip_plan_owned_pixels: the pixels that are a leaf of a retained cell (width * height unless the lattice has holes)."""
        return int(load_library().fri_hip_plan_owned_pixels(self._h))

    def set_stream_order(self, order=None):
        """fri_hip_plan_set_stream_order; order = None builds it with the host emitter library (frave_amd.emit.stream_order). Returns the order."""
        if order is None:
            from . import emit

            order = emit.stream_order(self.centers(), self.valid_mask())
        order = np.ascontiguousarray(order, np.uint32)
        _check(load_library().fri_hip_plan_set_stream_order(self._h, _p(order), order.size), "fri_hip_plan_set_stream_order", self.ctx)
        return order

    def symbol_stream_batch_dev(self, n_planes, d_coefs, coef_stride, d_bucket, d_prediction, out_stride, d_symbols, symbol_stride, stream=0):
        _check(load_library().fri_hip_symbol_stream_batch_dev(self._h, n_planes, d_coefs, coef_stride, d_bucket, d_prediction, out_stride, d_symbols, symbol_stride, stream),
               "fri_hip_symbol_stream_batch_dev", self.ctx)

    def encode_symbols_batch_dev(self, n_images, d_pixels, pixel_stride, qmatrix, fit, d_params, d_coefs, coef_stride, d_node_words, word_stride, d_symbols, symbol_stride,
                                 d_hist, d_oob, d_fit_range=0, stream=0):
        """fri_hip_encode_symbols_batch_dev: forward -> [fit] -> scan (halfword form) -> gather into stream order; everything in device memory, asynchronous.
        d_coefs = 0 / None: the coefficients stay inside the chain as the plan's compact int16 planes (same streams, histograms and parameters; faster);
        d_node_words = 0 / None as well: the scan writes the streams itself, no node words, no gather kernel (faster still)."""
        q = _q(qmatrix)
        _check(load_library().fri_hip_encode_symbols_batch_dev(self._h, n_images, d_pixels, pixel_stride, _p(q), 1 if fit else 0, d_params, d_coefs, coef_stride, d_node_words,
                                                               word_stride, d_symbols, symbol_stride, d_hist, d_oob, d_fit_range, stream), "fri_hip_encode_symbols_batch_dev", self.ctx)

    def set_dequantiser(self, multiply):
        """fri_hip_plan_set_dequantiser: False = the reference's dividing quantization::decode (default), True = coefficient x qmatrix[layer];
        or one of DEQUANT_REFERENCE, DEQUANT_MULTIPLY, DEQUANT_MIDPOINT (the middle of the truncating quantiser's interval)."""
        mode = (1 if multiply else 0) if isinstance(multiply, bool) else int(multiply)
        _check(load_library().fri_hip_plan_set_dequantiser(self._h, mode), "fri_hip_plan_set_dequantiser")

    def measure_distortion_dev(self, d_coefs, d_reference_pixels, d_out, qmatrix=None, stream=0):
        """fri_hip_measure_distortion_dev: K3 with the plan's dequantiser and colour transform compared with d_reference_pixels instead of written;
        d_out (uint64 [2 C + 1], device) = per channel c the sum of squared errors at 2 c and the largest absolute error at 2 c + 1, the owned pixels at 2 C."""
        q = _q(qmatrix)
        _check(load_library().fri_hip_measure_distortion_dev(self._h, d_coefs, _p(q), d_reference_pixels, d_out, stream), "fri_hip_measure_distortion_dev", self.ctx)

    def search_quality(self, pixels, target_db, stream=0):
        """fri_hip_search_quality (pixels: a host array) or fri_hip_search_quality_dev (pixels: a device pointer, an int): the lowest quality whose
        midpoint-dequantised round trip reaches target_db, by the bisection the header describes. Returns (quality, psnr_db)."""
        return _search(self, "fri_hip_search_quality", pixels, float(target_db), C.c_double, stream)

    def measure_ssim(self, a, b):
        """fri_hip_measure_ssim: the SSIM sums of two host rasters of the plan's shape (a the source, b the reconstruction) - int64 [C + 1], per channel
        the sum of the window values in units of 2^-32, then the window count (ssim_of turns them into SSIM)."""
        pa, pb = np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(b, np.uint8)
        assert pa.size == self.pixel_bytes and pb.size == self.pixel_bytes
        out = np.zeros(self.channels + 1, np.int64)
        _check(load_library().fri_hip_measure_ssim(self._h, _p(pa), _p(pb), _p(out)), "fri_hip_measure_ssim", self.ctx)
        return out

    def measure_ssim_dev(self, d_a, d_b, d_out, n_images=1, pixel_stride=0, stream=0):
        """fri_hip_measure_ssim_dev: K7 over n_images raster pairs (pair k at d_a / d_b + k pixel_stride bytes) into d_out (int64 [n_images][C + 1], device),
        which it zeroes on `stream` first; only enqueues."""
        _check(load_library().fri_hip_measure_ssim_dev(self._h, n_images, d_a, d_b, pixel_stride, d_out, stream), "fri_hip_measure_ssim_dev", self.ctx)

    def search_quality_ssim(self, pixels, target, stream=0):
        """fri_hip_search_quality_ssim (pixels: a host array) or its _dev form (pixels: a device pointer, an int): the lowest quality whose midpoint-dequantised
        round trip reaches an SSIM of target (0 < target <= 1), by the bisection of search_quality. Returns (quality, ssim); 100 means "code losslessly"."""
        return _search(self, "fri_hip_search_quality_ssim", pixels, float(target), C.c_double, stream)

    def estimate_size(self, hist, oob=None, stream=0, n_images=1, d_bytes=None, d_models=None):
        """The estimated .frv bytes of the histograms (include/fri_hip.h gives the formula); UINT64_MAX where the emitter would refuse the image.
        hist as a host array [C][10][1024] (oob [C] or None): fri_hip_estimate_size, returns an int. hist as a device pointer (an int, [n_images][C][10][1024];
        oob a device pointer or None): fri_hip_estimate_size_dev, which only enqueues on `stream` - d_bytes (uint64 [n_images]) and d_models (uint32
        [n_images][C][10][4] or None) are device pointers then, and the call returns None."""
        L = load_library()
        if isinstance(hist, int):
            assert d_bytes
            _check(L.fri_hip_estimate_size_dev(self._h, n_images, hist, oob or None, d_bytes, d_models or None, stream), "fri_hip_estimate_size_dev", self.ctx)
            return None
        h = np.ascontiguousarray(hist, np.uint32)
        assert h.size == self.channels * 10 * 1024
        o = None if oob is None else np.ascontiguousarray(oob, np.uint64)
        assert o is None or o.size == self.channels
        out = C.c_uint64(0)
        _check(L.fri_hip_estimate_size(self._h, _p(h), None if o is None else _p(o), C.byref(out)), "fri_hip_estimate_size", self.ctx)
        return out.value

    def search_quality_for_size(self, pixels, max_bytes, stream=0):
        """fri_hip_search_quality_for_size (pixels: a host array) or its _dev form (pixels: a device pointer, an int): the highest quality whose estimated
        file is at most max_bytes, by the bisection the header describes. Returns (quality, estimated bytes); FriHipError with code -7 when nothing fits."""
        return _search(self, "fri_hip_search_quality_for_size", pixels, int(max_bytes), C.c_uint64, stream)

    def set_colour_transform(self, mode):
        """fri_hip_plan_set_colour_transform: COLOUR_NONE (default), COLOUR_RCT or COLOUR_YCBCR (C = 3 plans): every forward entry point then codes the
        planes (Y, Cb, Cr) of the R, G, B pixels - (G, B - G + 128, R - G + 128) mod 256 for the RCT, the JFIF transform in 16-bit fixed point for YCbCr (lossy,
        include/fri_hip.h) - and every inverse entry point writes R, G, B back."""
        _check(load_library().fri_hip_plan_set_colour_transform(self._h, int(mode)), "fri_hip_plan_set_colour_transform")
        self.colour_transform = int(mode)

    def assume_forward_coefficients(self, on=True):
        """fri_hip_plan_assume_forward_coefficients: the predict entry points then skip the exact-kernel guard launch."""
        _check(load_library().fri_hip_plan_assume_forward_coefficients(self._h, 1 if on else 0), "fri_hip_plan_assume_forward_coefficients")

    # ---- getters -------------------------------------------------------------------------------
    def centers(self):
        out = np.empty((self.num_cells, 2), np.int32)
        _check(load_library().fri_hip_plan_centers(self._h, _p(out)), "fri_hip_plan_centers")
        return out

    def valid_mask(self):
        out = np.empty((self.num_cells, 16), np.uint32)
        _check(load_library().fri_hip_plan_valid_mask(self._h, _p(out)), "fri_hip_plan_valid_mask")
        return out

    def valid_bits(self):
        """bool [F][512] expansion of valid_mask()."""
        m = self.valid_mask()
        return ((m[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1).astype(bool).reshape(self.num_cells, 512)

    def neighbour_cells(self):
        out = np.empty((self.num_cells, 8), np.int32)
        _check(load_library().fri_hip_plan_neighbour_cells(self._h, _p(out)), "fri_hip_plan_neighbour_cells")
        return out

    def tiling(self):
        out = np.empty(8, np.int32)
        _check(load_library().fri_hip_plan_tiling(self._h, _p(out)), "fri_hip_plan_tiling")
        return dict(zip(("n_wg", "n_tiles", "lds_pitch", "lds_rows", "max_tile_cells", "band_rows", "cells_per_tile", "cells_per_wg"), (int(v) for v in out)))

    def predict_grid(self):
        """fri_hip_plan_predict_grid: the tiles K2 / K4 walk and the grid limits of their launchers (a host-only plan: the knobs, 0 where unset)."""
        out = np.zeros(4, np.uint32)
        _check(load_library().fri_hip_plan_predict_grid(self._h, _p(out)), "fri_hip_plan_predict_grid")
        return dict(zip(("n_pred_tiles", "pred_blocks", "hist_blocks", "k4_older_eighths"), (int(v) for v in out)))

    def pred_slots(self):
        """fri_hip_plan_pred_slots: int32 [n_pred_tiles][36], the 6 x 6 slot squares of the prediction tiles (cell id, | 0x40000000 for an interior cell, -1: none)."""
        out = np.empty((self.predict_grid()["n_pred_tiles"], 36), np.int32)
        _check(load_library().fri_hip_plan_pred_slots(self._h, _p(out)), "fri_hip_plan_pred_slots")
        return out

    def inverse_lists(self):
        out = np.zeros(5, np.uint64)
        _check(load_library().fri_hip_plan_inverse_lists(self._h, _p(out)), "fri_hip_plan_inverse_lists")
        return dict(zip(("built", "quads", "dwords", "part_bytes", "rect_bytes"), (int(v) for v in out)))

    def read_trace(self):
        """[n_wg, 16] uint64 time stamps (100 MHz ticks) of the last forward/inverse launch; needs FRI_HIP_TRACE=1 at plan creation."""
        out = np.zeros((self.tiling()["n_wg"], 16), np.uint64)
        _check(load_library().fri_hip_plan_read_trace(self._h, _p(out)), "fri_hip_plan_read_trace", self.ctx)
        return out

    def tile_table(self):
        t = self.tiling()
        tiles = np.empty((t["n_tiles"], 6), np.int32)
        cells = np.empty(self.num_cells, np.int32)
        wg = np.empty(t["n_wg"] + 1, np.int32)
        _check(load_library().fri_hip_plan_tile_table(self._h, _p(tiles), _p(cells), _p(wg)), "fri_hip_plan_tile_table")
        return tiles, cells, wg

    def neighbour_table(self):
        out = np.empty((512, 6), np.uint16)
        _check(load_library().fri_hip_plan_neighbour_table(self._h, _p(out)), "fri_hip_plan_neighbour_table")
        return out

    # ---- host-pointer entry points -------------------------------------------------------------
    def transform_quant(self, pixels, qmatrix=None):
        px = np.ascontiguousarray(pixels, np.uint8).reshape(-1)
        assert px.size == self.pixel_bytes
        out = np.empty((self.channels, self.num_cells, 512), np.int32)
        q = _q(qmatrix)
        _check(load_library().fri_hip_transform_quant(self._h, _p(px), _p(q), _p(out)), "fri_hip_transform_quant", self.ctx)
        return out

    def transform_quant_batch(self, images, qmatrix=None):
        imgs = [np.ascontiguousarray(i, np.uint8).reshape(-1) for i in images]
        outs = [np.empty((self.channels, self.num_cells, 512), np.int32) for _ in imgs]
        n = len(imgs)
        pin = (C.c_void_p * n)(*[i.ctypes.data for i in imgs])
        pout = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        q = _q(qmatrix)
        _check(load_library().fri_hip_transform_quant_batch(self._h, n, pin, _p(q), pout), "fri_hip_transform_quant_batch", self.ctx)
        return outs

    def encode_image_batch(self, images, qmatrix=None, fit=True, params=None, want_bucket=True, want_prediction=True):
        """fri_hip_encode_image_batch: the per-image encode loop for host buffers on this plan's device (lists per image, as Multi.encode_image)."""
        return _encode_batch(load_library().fri_hip_encode_image_batch, self._h, "fri_hip_encode_image_batch", self.ctx, images, self.channels, self.num_cells, qmatrix, fit, params,
                             want_bucket, want_prediction)

    def predict_histogram(self, coefs, channel, value_params, width_params, want_bucket=True, want_prediction=True):
        """(bucket, prediction, hist, n_out_of_alphabet); an output that is not wanted is passed as NULL and returned as None."""
        co = np.ascontiguousarray(coefs, np.int32)
        assert co.size == self.coef_count
        vp = np.ascontiguousarray(value_params, np.float32).reshape(3, 6)
        wp = np.ascontiguousarray(width_params, np.float32).reshape(3, 6)
        bucket = np.empty((self.num_cells, 512), np.uint8) if want_bucket else None
        pred = np.empty((self.num_cells, 512), np.int32) if want_prediction else None
        hist = np.empty((10, 1024), np.uint32)
        oob = C.c_uint64(0)
        _check(load_library().fri_hip_predict_histogram(self._h, _p(co), channel, _p(vp), _p(wp), _p(bucket) if want_bucket else None,
                                                        _p(pred) if want_prediction else None, _p(hist), C.addressof(oob)),
               "fri_hip_predict_histogram", self.ctx)
        return bucket, pred, hist, oob.value

    def fit_value_sums(self, coefs, channel):
        """gram[3][7][7] (full symmetric int64) of u = [v0..v5, value] per layer group."""
        co = np.ascontiguousarray(coefs, np.int32)
        assert co.size == self.coef_count
        tri = np.empty((3, 28), np.int64)
        _check(load_library().fri_hip_fit_value_sums(self._h, _p(co), channel, _p(tri)), "fri_hip_fit_value_sums", self.ctx)
        return _untriangle(tri, 7)

    def fit_width_sums(self, coefs, channel, value_params):
        """(wtw[3][6][6] int64 over the Some rows, wtr[3][6] float64, rows[3])."""
        co = np.ascontiguousarray(coefs, np.int32)
        assert co.size == self.coef_count
        vp = np.ascontiguousarray(value_params, np.float32).reshape(3, 6)
        tri = np.empty((3, 21), np.int64)
        wtr = np.empty((3, 6), np.float64)
        rows = np.empty(3, np.uint64)
        _check(load_library().fri_hip_fit_width_sums(self._h, _p(co), channel, _p(vp), _p(tri), _p(wtr), _p(rows)), "fri_hip_fit_width_sums", self.ctx)
        return _untriangle(tri, 6), wtr, rows

    def inverse_transform(self, coefs, qmatrix=None):
        co = np.ascontiguousarray(coefs, np.int32)
        assert co.size == self.coef_count
        out = np.empty(self.pixel_bytes, np.uint8)
        q = _q(qmatrix)
        _check(load_library().fri_hip_inverse_transform(self._h, _p(co), _p(q), _p(out)), "fri_hip_inverse_transform", self.ctx)
        return out

    # ---- device-pointer entry points (pointers are ints, e.g. torch.Tensor.data_ptr()) ---------
    def transform_quant_dev(self, d_pixels, d_coefs, qmatrix=None, stream=0, n_images=1, pixel_stride=0, coef_stride=0):
        q = _q(qmatrix)
        _check(load_library().fri_hip_transform_quant_batch_dev(self._h, n_images, d_pixels, pixel_stride, _p(q), d_coefs, coef_stride, stream),
               "fri_hip_transform_quant_batch_dev", self.ctx)

    def predict_histogram_dev(self, d_coefs, channel, value_params, width_params, d_bucket, d_prediction, d_hist, d_oob, stream=0):
        vp = np.ascontiguousarray(value_params, np.float32).reshape(3, 6)
        wp = np.ascontiguousarray(width_params, np.float32).reshape(3, 6)
        _check(load_library().fri_hip_predict_histogram_dev(self._h, d_coefs, channel, _p(vp), _p(wp), d_bucket, d_prediction, d_hist, d_oob, stream),
               "fri_hip_predict_histogram_dev", self.ctx)

    def fit_value_sums_dev(self, d_coefs, channel, d_gram, stream=0):
        _check(load_library().fri_hip_fit_value_sums_dev(self._h, d_coefs, channel, d_gram, stream), "fri_hip_fit_value_sums_dev", self.ctx)

    def fit_width_sums_dev(self, d_coefs, channel, value_params, d_wtw, d_wtr, stream=0):
        vp = np.ascontiguousarray(value_params, np.float32).reshape(3, 6)
        _check(load_library().fri_hip_fit_width_sums_dev(self._h, d_coefs, channel, _p(vp), d_wtw, d_wtr, stream), "fri_hip_fit_width_sums_dev", self.ctx)

    def encode_image(self, pixels, qmatrix=None, fit=True, value_params=None, width_params=None, want_bucket=True, want_prediction=True):
        """fri_hip_encode_image: (coefs [C][F][512], value_params [C][3][6], width_params [C][3][6], bucket, prediction, hist [C][10][1024], oob [C])."""
        px = np.ascontiguousarray(pixels, np.uint8).reshape(-1)
        assert px.size == self.pixel_bytes
        c, f = self.channels, self.num_cells
        vp = np.zeros((c, 3, 6), np.float32) if value_params is None else np.ascontiguousarray(value_params, np.float32).reshape(c, 3, 6).copy()
        wp = np.zeros((c, 3, 6), np.float32) if width_params is None else np.ascontiguousarray(width_params, np.float32).reshape(c, 3, 6).copy()
        coefs = np.empty((c, f, 512), np.int32)
        bucket = np.empty((c, f, 512), np.uint8) if want_bucket else None
        pred = np.empty((c, f, 512), np.int32) if want_prediction else None
        hist = np.empty((c, 10, 1024), np.uint32)
        oob = np.zeros(c, np.uint64)
        q = _q(qmatrix)
        _check(load_library().fri_hip_encode_image(self._h, _p(px), _p(q), 1 if fit else 0, _p(vp), _p(wp), _p(coefs), _p(bucket) if want_bucket else None,
                                                   _p(pred) if want_prediction else None, _p(hist), _p(oob)), "fri_hip_encode_image", self.ctx)
        return coefs, vp, wp, bucket, pred, hist, oob

    def encode_image_symbols(self, pixels, qmatrix=None, fit=True, value_params=None, width_params=None):
        """fri_hip_encode_image_symbols: (symbols uint16 [C][num_some], value_params, width_params, hist [C][10][1024], oob [C]); needs set_stream_order()."""
        px = np.ascontiguousarray(pixels, np.uint8).reshape(-1)
        assert px.size == self.pixel_bytes
        c = self.channels
        vp = np.zeros((c, 3, 6), np.float32) if value_params is None else np.ascontiguousarray(value_params, np.float32).reshape(c, 3, 6).copy()
        wp = np.zeros((c, 3, 6), np.float32) if width_params is None else np.ascontiguousarray(width_params, np.float32).reshape(c, 3, 6).copy()
        sym = np.empty((c, self.num_some), np.uint16)
        hist = np.empty((c, 10, 1024), np.uint32)
        oob = np.zeros(c, np.uint64)
        q = _q(qmatrix)
        _check(load_library().fri_hip_encode_image_symbols(self._h, _p(px), _p(q), 1 if fit else 0, _p(vp), _p(wp), _p(sym), _p(hist), _p(oob)), "fri_hip_encode_image_symbols", self.ctx)
        return sym, vp, wp, hist, oob

    def predict_image(self, coefs, fit=True, value_params=None, width_params=None):
        """fri_hip_predict_image: (value_params, width_params, bucket [C][F][512], prediction, hist [C][10][1024], oob [C])."""
        co = np.ascontiguousarray(coefs, np.int32)
        assert co.size == self.coef_count
        c, f = self.channels, self.num_cells
        vp = np.zeros((c, 3, 6), np.float32) if value_params is None else np.ascontiguousarray(value_params, np.float32).reshape(c, 3, 6).copy()
        wp = np.zeros((c, 3, 6), np.float32) if width_params is None else np.ascontiguousarray(width_params, np.float32).reshape(c, 3, 6).copy()
        bucket, pred = np.empty((c, f, 512), np.uint8), np.empty((c, f, 512), np.int32)
        hist, oob = np.empty((c, 10, 1024), np.uint32), np.zeros(c, np.uint64)
        _check(load_library().fri_hip_predict_image(self._h, _p(co), 1 if fit else 0, _p(vp), _p(wp), _p(bucket), _p(pred), _p(hist), _p(oob)), "fri_hip_predict_image", self.ctx)
        return vp, wp, bucket, pred, hist, oob

    def encode_image_dev(self, d_pixels, d_coefs, d_bucket, d_prediction, d_hist, d_oob, value_params, width_params, fit=False, qmatrix=None, stream=0):
        """fri_hip_encode_image_dev; value_params / width_params are float32 [C][3][6] numpy arrays (in, or out when fit)."""
        q = _q(qmatrix)
        assert value_params.dtype == np.float32 and width_params.dtype == np.float32 and value_params.size == width_params.size == self.channels * 18
        _check(load_library().fri_hip_encode_image_dev(self._h, d_pixels, _p(q), 1 if fit else 0, _p(value_params), _p(width_params), d_coefs, d_bucket, d_prediction,
                                                       d_hist, d_oob, stream), "fri_hip_encode_image_dev", self.ctx)

    def predict_histogram_batch_dev(self, n_planes, d_coefs, coef_stride, d_params, d_bucket, d_prediction, out_stride, d_hist, d_oob, stream=0):
        _check(load_library().fri_hip_predict_histogram_batch_dev(self._h, n_planes, d_coefs, coef_stride, d_params, d_bucket, d_prediction, out_stride, d_hist, d_oob,
                                                                  stream), "fri_hip_predict_histogram_batch_dev", self.ctx)

    def fit_value_sums_batch_dev(self, n_planes, d_coefs, coef_stride, d_gram, stream=0):
        _check(load_library().fri_hip_fit_value_sums_batch_dev(self._h, n_planes, d_coefs, coef_stride, d_gram, stream), "fri_hip_fit_value_sums_batch_dev", self.ctx)

    def fit_width_sums_batch_dev(self, n_planes, d_coefs, coef_stride, d_params, d_wtw, d_wtr, stream=0):
        _check(load_library().fri_hip_fit_width_sums_batch_dev(self._h, n_planes, d_coefs, coef_stride, d_params, d_wtw, d_wtr, stream),
               "fri_hip_fit_width_sums_batch_dev", self.ctx)

    def fit_value_params_batch_dev(self, n_planes, d_gram, d_params, stream=0):
        _check(load_library().fri_hip_fit_value_params_batch_dev(self._h, n_planes, d_gram, d_params, stream), "fri_hip_fit_value_params_batch_dev", self.ctx)

    def fit_width_params_batch_dev(self, n_planes, d_wtw, d_wtr, d_params, stream=0):
        _check(load_library().fri_hip_fit_width_params_batch_dev(self._h, n_planes, d_wtw, d_wtr, d_params, stream), "fri_hip_fit_width_params_batch_dev", self.ctx)

    def fit_params_batch_dev(self, n_planes, d_coefs, coef_stride, d_params, d_fit_out_of_range=None, stream=0):
        """fri_hip_fit_params_batch_dev: the whole fit (sums + 6 x 6 solves) of n_planes planes on the device, parameters into d_params."""
        _check(load_library().fri_hip_fit_params_batch_dev(self._h, n_planes, d_coefs, coef_stride, d_params, d_fit_out_of_range, stream),
               "fri_hip_fit_params_batch_dev", self.ctx)

    def encode_image_batch_dev(self, n_images, d_pixels, pixel_stride, d_params, d_coefs, coef_stride, d_bucket, d_prediction, out_stride, d_hist, d_oob,
                               fit=True, d_fit_out_of_range=None, qmatrix=None, stream=0):
        """fri_hip_encode_image_batch_dev: K1 -> (fit) -> K2 for n_images images, all in device memory, nothing but enqueues."""
        q = _q(qmatrix)
        _check(load_library().fri_hip_encode_image_batch_dev(self._h, n_images, d_pixels, pixel_stride, _p(q), 1 if fit else 0, d_params, d_coefs, coef_stride,
                                                             d_bucket, d_prediction, out_stride, d_hist, d_oob, d_fit_out_of_range, stream),
               "fri_hip_encode_image_batch_dev", self.ctx)

    def inverse_transform_batch_dev(self, n_images, d_coefs, coef_stride, d_pixels, pixel_stride, qmatrix=None, stream=0):
        q = _q(qmatrix)
        _check(load_library().fri_hip_inverse_transform_batch_dev(self._h, n_images, d_coefs, coef_stride, _p(q), d_pixels, pixel_stride, stream),
               "fri_hip_inverse_transform_batch_dev", self.ctx)

    def inverse_transform_dev(self, d_coefs, d_pixels, qmatrix=None, stream=0):
        q = _q(qmatrix)
        _check(load_library().fri_hip_inverse_transform_dev(self._h, d_coefs, _p(q), d_pixels, stream), "fri_hip_inverse_transform_dev", self.ctx)

    def tune_forward(self, launches=0):
        """fri_hip_plan_tune_forward: measure candidate tilings of the forward kernel on this device and keep the fastest. Returns the report (dict)."""
        import json

        buf = C.create_string_buffer(16384)
        _check(load_library().fri_hip_plan_tune_forward(self._h, launches, buf, len(buf)), "fri_hip_plan_tune_forward", self.ctx)
        try:
            return json.loads(buf.value.decode() or "{}")
        except ValueError:  # a report cut short by the buffer
            return {"raw": buf.value.decode(errors="replace")}

    def time_transform_quant_streams_dev(self, n_images, d_pixels, pixel_stride, d_coefs, coef_stride, iters, n_streams, qmatrix=None):
        q = _q(qmatrix)
        us = C.c_double(0)
        _check(load_library().fri_hip_time_transform_quant_streams_dev(self._h, n_images, d_pixels, pixel_stride, _p(q), d_coefs, coef_stride, iters, n_streams,
                                                                       C.byref(us)), "fri_hip_time_transform_quant_streams_dev", self.ctx)
        return us.value

    def time_transform_quant_dev(self, n_images, d_pixels, pixel_stride, d_coefs, coef_stride, iters, qmatrix=None, stream=0):
        q = _q(qmatrix)
        us = C.c_double(0)
        _check(load_library().fri_hip_time_transform_quant_dev(self._h, n_images, d_pixels, pixel_stride, _p(q), d_coefs, coef_stride, iters, stream,
                                                               C.byref(us)), "fri_hip_time_transform_quant_dev", self.ctx)
        return us.value


class Plan420:
    """fri_hip_plan420: lossy YCbCr coding with 4:2:0 chroma subsampling (include/fri_hip.h has the format). Owns two ordinary C = 1 plans, .luma (W x H) and
    .chroma (cw x ch; Cb and Cr are planes 0 and 1 of a batch) - Plan views that do not own their handle and die with this object. ctx=None gives a
    host-only plan (getters only)."""

    def __init__(self, ctx, width, height):
        self._h = None
        self.ctx = ctx
        self.width, self.height = width, height
        self.cw, self.ch = (width + 1) // 2, (height + 1) // 2
        h = C.c_void_p()
        L = load_library()
        _check(L.fri_hip_plan420_create(ctx._h if ctx else None, width, height, C.byref(h)), "fri_hip_plan420_create", ctx)
        self._h = h
        self.luma = Plan(ctx, width, height, 1, _handle=L.fri_hip_plan420_luma(h))
        self.chroma = Plan(ctx, self.cw, self.ch, 1, _handle=L.fri_hip_plan420_chroma(h))
        self.pixel_bytes = 3 * width * height
        self.plane_bytes = width * height + 2 * self.cw * self.ch
        self.num_symbols = self.luma.num_some + 2 * self.chroma.num_some
        self.coef_count = (self.luma.num_cells + 2 * self.chroma.num_cells) * 512

    def close(self):
        if self._h:
            self.luma.close()
            self.chroma.close()
            load_library().fri_hip_plan420_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream_order(self):
        """fri_hip_plan_set_stream_order on both inner plans (encode_image420_symbols needs it)."""
        self.luma.set_stream_order()
        self.chroma.set_stream_order()

    # ---- device-pointer entry points (pointers are ints) --------------------------------------------
    def split420_dev(self, d_rgb, d_y, d_cbcr, stream=0):
        """fri_hip_split420_dev: R, G, B [H][W][3] -> Y [H][W] and Cb, Cr [ch][cw] each (contiguous); only enqueues."""
        _check(load_library().fri_hip_split420_dev(self._h, d_rgb, d_y, d_cbcr, stream), "fri_hip_split420_dev", self.ctx)

    def merge420_dev(self, d_y, d_cbcr, d_rgb, stream=0):
        """fri_hip_merge420_dev: the three planes -> R, G, B with the chroma planes upsampled by the (3, 1) / 4 triangle filter; only enqueues."""
        _check(load_library().fri_hip_merge420_dev(self._h, d_y, d_cbcr, d_rgb, stream), "fri_hip_merge420_dev", self.ctx)

    def measure_distortion420_dev(self, d_y, d_cbcr, d_reference_rgb, d_out, stream=0):
        """fri_hip_measure_distortion420_dev: the merge compared with d_reference_rgb instead of written; d_out uint64 [7] (device) as
        Plan.measure_distortion_dev at C = 3, d_out[6] = W H."""
        _check(load_library().fri_hip_measure_distortion420_dev(self._h, d_y, d_cbcr, d_reference_rgb, d_out, stream), "fri_hip_measure_distortion420_dev", self.ctx)

    # ---- host-pointer entry points ----------------------------------------------------------------
    def encode_image420_symbols(self, pixels, quality):
        """fri_hip_encode_image420_symbols: (symbols uint16 [n_y + 2 n_c] = Y, Cb, Cr streams, value_params [3][3][6], width_params [3][3][6],
        hist [3][10][1024], oob [3]); needs set_stream_order()."""
        px = np.ascontiguousarray(pixels, np.uint8).reshape(-1)
        assert px.size == self.pixel_bytes
        vp, wp = np.zeros((3, 3, 6), np.float32), np.zeros((3, 3, 6), np.float32)
        sym = np.empty(self.num_symbols, np.uint16)
        hist = np.empty((3, 10, 1024), np.uint32)
        oob = np.zeros(3, np.uint64)
        _check(load_library().fri_hip_encode_image420_symbols(self._h, _p(px), int(quality), _p(vp), _p(wp), _p(sym), _p(hist), _p(oob)),
               "fri_hip_encode_image420_symbols", self.ctx)
        return sym, vp, wp, hist, oob

    def decode_image420(self, coefs, quality):
        """fri_hip_decode_image420: coefs int32 = Y [F_y][512], Cb [F_c][512], Cr [F_c][512] (flat) -> pixels uint8 [H * W * 3]."""
        co = np.ascontiguousarray(coefs, np.int32).reshape(-1)
        assert co.size == self.coef_count
        out = np.empty(self.pixel_bytes, np.uint8)
        _check(load_library().fri_hip_decode_image420(self._h, _p(co), int(quality), _p(out)), "fri_hip_decode_image420", self.ctx)
        return out

    def search_quality(self, pixels, target_db, stream=0):
        """fri_hip_search_quality420[_dev] (pixels: a host array or a device pointer): (quality, RGB PSNR in dB); 100 = code losslessly."""
        return _search(self, "fri_hip_search_quality420", pixels, float(target_db), C.c_double, stream)

    def search_quality_ssim(self, pixels, target, stream=0):
        """fri_hip_search_quality_ssim420[_dev]: (quality, RGB SSIM); 100 = code losslessly."""
        return _search(self, "fri_hip_search_quality_ssim420", pixels, float(target), C.c_double, stream)

    def search_quality_for_size(self, pixels, max_bytes, stream=0):
        """fri_hip_search_quality_for_size420[_dev]: (quality, estimated bytes); FriHipError with code -7 when nothing fits."""
        return _search(self, "fri_hip_search_quality_for_size420", pixels, int(max_bytes), C.c_uint64, stream)


class PlanRGBA:
    """fri_hip_plan_rgba: RGBA coding - the colour as any C = 3 image, the alpha plane losslessly as a C = 1 image (include/fri_hip.h has the format). Owns two
    ordinary plans on the same W x H lattice, .colour (C = 3: set the colour transform and the dequantiser of a decode here) and .alpha (C = 1) - Plan views that do
    not own their handle and die with this object. ctx=None gives a host-only plan (getters only). Calls on one PlanRGBA must be ordered on one stream: they share
    the plan's staging buffers."""

    def __init__(self, ctx, width, height):
        self._h = None
        self.ctx = ctx
        self.width, self.height = width, height
        h = C.c_void_p()
        L = load_library()
        _check(L.fri_hip_plan_rgba_create(ctx._h if ctx else None, width, height, C.byref(h)), "fri_hip_plan_rgba_create", ctx)
        self._h = h
        self.colour = Plan(ctx, width, height, 3, _handle=L.fri_hip_plan_rgba_colour(h))
        self.alpha = Plan(ctx, width, height, 1, _handle=L.fri_hip_plan_rgba_alpha(h))
        self.pixel_bytes = 4 * width * height
        self.num_cells = self.colour.num_cells
        self.num_some = self.colour.num_some  # symbols per channel, the same for all four
        self.coef_count = 4 * self.num_cells * 512

    def close(self):
        if self._h:
            self.colour.close()
            self.alpha.close()
            load_library().fri_hip_plan_rgba_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream_order(self):
        """fri_hip_plan_set_stream_order on both inner plans (the encodes need it)."""
        self.colour.set_stream_order()
        self.alpha.set_stream_order()

    # ---- device-pointer entry points (pointers are ints) --------------------------------------------
    def split_rgba_dev(self, d_rgba, d_rgb, d_a, clean=ALPHA_KEEP, stream=0):
        """fri_hip_split_rgba_dev: R, G, B, A [H][W][4] -> R, G, B [H][W][3] and A [H][W] (contiguous); ALPHA_CLEAN zeroes the colour where A == 0; only enqueues."""
        _check(load_library().fri_hip_split_rgba_dev(self._h, d_rgba, int(clean), d_rgb, d_a, stream), "fri_hip_split_rgba_dev", self.ctx)

    def merge_rgba_dev(self, d_rgb, d_a, d_rgba, stream=0):
        """fri_hip_merge_rgba_dev: the inverse interleave; only enqueues."""
        _check(load_library().fri_hip_merge_rgba_dev(self._h, d_rgb, d_a, d_rgba, stream), "fri_hip_merge_rgba_dev", self.ctx)

    def encode_symbols_rgba_dev(self, d_rgba, d_params, d_symbols, d_hist, d_oob, d_fit_out_of_range=None, clean=ALPHA_KEEP, qmatrix=None, fit=True, stream=0):
        """fri_hip_encode_symbols_rgba_dev: the split and the direct stream chain on both inner plans, everything on the device: d_params float32 [4][2][3][6],
        d_symbols uint16 [4][num_some], d_hist uint32 [4][10][1024], d_oob uint64 [4], d_fit_out_of_range uint64 [4] or None - the colour channels, then alpha.
        qmatrix is the colour's; alpha always takes ones. Needs set_stream_order()."""
        _check(load_library().fri_hip_encode_symbols_rgba_dev(self._h, d_rgba, int(clean), _p(_q(qmatrix)), int(bool(fit)), d_params, d_symbols, d_hist, d_oob,
                                                             d_fit_out_of_range, stream), "fri_hip_encode_symbols_rgba_dev", self.ctx)

    # ---- host-pointer entry points ----------------------------------------------------------------
    def encode_image_rgba_symbols(self, pixels, qmatrix=None, clean=ALPHA_KEEP):
        """fri_hip_encode_image_rgba_symbols: (symbols uint16 [4][num_some], value_params [4][3][6], width_params [4][3][6], hist [4][10][1024], oob [4]) - the
        colour channels, coded with qmatrix and the colour plan's transform, then the alpha plane, coded with ones; the fit is on. Needs set_stream_order()."""
        px = np.ascontiguousarray(pixels, np.uint8).reshape(-1)
        assert px.size == self.pixel_bytes
        vp, wp = np.zeros((4, 3, 6), np.float32), np.zeros((4, 3, 6), np.float32)
        sym = np.empty((4, self.num_some), np.uint16)
        hist = np.empty((4, 10, 1024), np.uint32)
        oob = np.zeros(4, np.uint64)
        _check(load_library().fri_hip_encode_image_rgba_symbols(self._h, _p(px), int(clean), _p(_q(qmatrix)), _p(vp), _p(wp), _p(sym), _p(hist), _p(oob)),
               "fri_hip_encode_image_rgba_symbols", self.ctx)
        return sym, vp, wp, hist, oob

    def decode_image_rgba(self, coefs, qmatrix=None):
        """fri_hip_decode_image_rgba: coefs int32 [4][F][512] (what emit.decode_image returns for a file with alpha) -> pixels uint8 [H * W * 4]. The colour planes
        go through the inverse kernel with qmatrix and the colour plan's transform and dequantiser, the alpha plane with ones."""
        co = np.ascontiguousarray(coefs, np.int32).reshape(-1)
        assert co.size == self.coef_count
        out = np.empty(self.pixel_bytes, np.uint8)
        _check(load_library().fri_hip_decode_image_rgba(self._h, _p(co), _p(_q(qmatrix)), _p(out)), "fri_hip_decode_image_rgba", self.ctx)
        return out


class PlanTiled:
    """fri_hip_plan_tiled: an image as a batch of independently coded tiles (include/fri_hip.h has the format). Owns one ordinary plan of the tile's shape, .tile -
    a Plan view that does not own its handle and dies with this object: set the colour transform, the dequantiser and the stream order there. ctx=None gives a
    host-only plan (getters only). flags: TILED_ALLOW_HOLES accepts a tile shape whose lattice does not own every pixel. Calls on one PlanTiled must be ordered on
    one stream: they share the plan's staging buffers."""

    def __init__(self, ctx, width, height, channels, tile_w, tile_h, flags=0):
        self._h = None
        self.ctx = ctx
        self.width, self.height, self.channels = width, height, channels
        h = C.c_void_p()
        L = load_library()
        _check(L.fri_hip_plan_tiled_create(ctx._h if ctx else None, width, height, channels, tile_w, tile_h, flags, C.byref(h)), "fri_hip_plan_tiled_create", ctx)
        self._h = h
        self.tile = Plan(ctx, tile_w, tile_h, channels, _handle=L.fri_hip_plan_tiled_tile(h))
        grid = np.zeros(4, np.uint32)
        _check(L.fri_hip_plan_tiled_grid(h, _p(grid)), "fri_hip_plan_tiled_grid", ctx)
        self.nx, self.ny, self.tile_w, self.tile_h = (int(v) for v in grid)
        self.n_tiles = self.nx * self.ny
        self.pixel_bytes = width * height * channels
        self.tile_bytes = self.n_tiles * tile_w * tile_h * channels  # the tile raster [ny nx][tile_h][tile_w][C]
        self.num_cells = self.tile.num_cells
        self.num_some = self.tile.num_some  # symbols per channel of one tile
        self.coef_count = self.n_tiles * channels * self.num_cells * 512

    def close(self):
        if self._h:
            self.tile.close()
            load_library().fri_hip_plan_tiled_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream_order(self):
        """fri_hip_plan_set_stream_order on the inner plan (the encodes need it)."""
        return self.tile.set_stream_order()

    # ---- device-pointer entry points (pointers are ints) --------------------------------------------
    def split_tiles_dev(self, d_raster, d_tiles, stream=0):
        """fri_hip_split_tiles_dev: [H][W][C] -> [ny nx][tile_h][tile_w][C] with edge replication; only enqueues."""
        _check(load_library().fri_hip_split_tiles_dev(self._h, d_raster, d_tiles, stream), "fri_hip_split_tiles_dev", self.ctx)

    def merge_tiles_dev(self, d_tiles, d_raster, stream=0):
        """fri_hip_merge_tiles_dev: the tile raster's in-image pixels back into [H][W][C]; only enqueues."""
        _check(load_library().fri_hip_merge_tiles_dev(self._h, d_tiles, d_raster, stream), "fri_hip_merge_tiles_dev", self.ctx)

    def encode_symbols_tiled_dev(self, d_raster, d_params, d_symbols, d_hist, d_oob, d_fit_out_of_range=None, qmatrix=None, fit=True, stream=0):
        """fri_hip_encode_symbols_tiled_dev: the split and one direct stream chain over all tiles, everything on the device: d_params float32
        [n_tiles][C][2][3][6], d_symbols uint16 [n_tiles][C][num_some], d_hist uint32 [n_tiles][C][10][1024], d_oob uint64 [n_tiles][C], d_fit_out_of_range uint64
        [n_tiles][C] or None. Needs set_stream_order()."""
        _check(load_library().fri_hip_encode_symbols_tiled_dev(self._h, d_raster, _p(_q(qmatrix)), int(bool(fit)), d_params, d_symbols, d_hist, d_oob, d_fit_out_of_range,
                                                              stream), "fri_hip_encode_symbols_tiled_dev", self.ctx)

    # ---- host-pointer entry points ----------------------------------------------------------------
    def encode_image_tiled_symbols(self, pixels, qmatrix=None):
        """fri_hip_encode_image_tiled_symbols: (symbols uint16 [n_tiles][C][num_some], value_params [n_tiles][C][3][6], width_params [n_tiles][C][3][6], hist
        [n_tiles][C][10][1024], oob [n_tiles][C]) - what emit.tiled_encode_from_streams takes; the fit is on. Needs set_stream_order()."""
        px = np.ascontiguousarray(pixels, np.uint8).reshape(-1)
        assert px.size == self.pixel_bytes
        n, c = self.n_tiles, self.channels
        vp, wp = np.zeros((n, c, 3, 6), np.float32), np.zeros((n, c, 3, 6), np.float32)
        sym = np.empty((n, c, self.num_some), np.uint16)
        hist = np.empty((n, c, 10, 1024), np.uint32)
        oob = np.zeros((n, c), np.uint64)
        _check(load_library().fri_hip_encode_image_tiled_symbols(self._h, _p(px), _p(_q(qmatrix)), _p(vp), _p(wp), _p(sym), _p(hist), _p(oob)),
               "fri_hip_encode_image_tiled_symbols", self.ctx)
        return sym, vp, wp, hist, oob

    def encode_image_tiled_coded(self, pixels, qmatrix=None, word_stride=None):
        """fri_hip_encode_image_tiled_coded: the tiled chain with the fit, then the device rANS coder - (words uint32 [n_tiles C][word_stride], n_words uint32
        [n_tiles C], models uint32 [n_tiles C][10][4], off_values uint16 [n_tiles C][10][1024], status uint32 [n_tiles C][4], value_params, width_params
        [n_tiles][C][3][6]): what emit.tiled_encode_from_coded takes. word_stride: words per plane of the returned array (default num_some + 20, which always
        suffices). Needs set_stream_order()."""
        px = np.ascontiguousarray(pixels, np.uint8).reshape(-1)
        assert px.size == self.pixel_bytes
        n, c = self.n_tiles, self.channels
        planes = n * c
        stride = self.num_some + 20 if word_stride is None else int(word_stride)
        vp, wp = np.zeros((n, c, 3, 6), np.float32), np.zeros((n, c, 3, 6), np.float32)
        words = np.zeros((planes, stride), np.uint32)
        n_words, models = np.zeros(planes, np.uint32), np.zeros((planes, 10, 4), np.uint32)
        off, status = np.zeros((planes, 10, 1024), np.uint16), np.zeros((planes, 4), np.uint32)
        _check(load_library().fri_hip_encode_image_tiled_coded(self._h, _p(px), _p(_q(qmatrix)), _p(vp), _p(wp), _p(words), stride, _p(n_words), _p(models), _p(off), _p(status)),
               "fri_hip_encode_image_tiled_coded", self.ctx)
        return words, n_words, models, off, status, vp, wp

    def decode_image_tiled(self, coefs, qmatrix=None):
        """fri_hip_decode_image_tiled: coefs int32 [n_tiles][C][F][512] (what emit.tiled_decode returns) -> pixels uint8 [H * W * C], through the inverse kernel with
        qmatrix and the inner plan's colour transform and dequantiser, then the merge."""
        co = np.ascontiguousarray(coefs, np.int32).reshape(-1)
        assert co.size == self.coef_count
        out = np.empty(self.pixel_bytes, np.uint8)
        _check(load_library().fri_hip_decode_image_tiled(self._h, _p(co), _p(_q(qmatrix)), _p(out)), "fri_hip_decode_image_tiled", self.ctx)
        return out

    def decode_coded(self, coded, qmatrix=None):
        """fri_hip_decode_image_tiled_coded: the coded planes of a `frit` file - what emit.tiled_parse_coded returns, with or without its TiledInfo - through the
        device decoder (K13), the inverse kernel and the merge -> (pixels uint8 [H * W * C], status uint32 [n_tiles C][4]); the pixels are decode_image_tiled's of
        emit.tiled_decode's planes. A plane the decoder refuses raises FriHipError (-1) with the status as .status. Needs set_stream_order()."""
        planes = self.n_tiles * self.channels
        words, n_words, models, off, vp, wp = _coded_planes(coded, planes)
        out, status = np.empty(self.pixel_bytes, np.uint8), np.zeros((planes, 4), np.uint32)
        rc = load_library().fri_hip_decode_image_tiled_coded(self._h, _p(words), words.shape[1], _p(n_words), _p(models), _p(off), _p(vp), _p(wp), _p(_q(qmatrix)), _p(out),
                                                             _p(status))
        _check_decode(rc, "fri_hip_decode_image_tiled_coded", self.ctx, status)
        return out, status

    # ---- preview decode: stop at a level, write a thumbnail (K14) ---------------------------------------
    def preview_tiles_dev(self, d_coefs, coef_stride, node_stride, levels, shift, d_out, qmatrix=None, stream=0):
        """fri_hip_preview_tiles_dev (K14), device pointers as ints: planes [n_tiles][C] coef_stride elements apart, node h of cell k at k * node_stride + h
        (node_stride 512 or 2^levels) -> d_out uint8 [h'][w'][C], any alignment. Only enqueues; capturable."""
        _check(load_library().fri_hip_preview_tiles_dev(self._h, d_coefs, coef_stride, node_stride, int(levels), int(shift), _p(_q(qmatrix)), d_out, stream),
               "fri_hip_preview_tiles_dev", self.ctx)

    def preview(self, coefs, levels, shift, qmatrix=None):
        """fri_hip_preview_image_tiled: the compact planes int32 [n_tiles][C][F][2^levels] (what emit.tiled_decode_levels returns) -> the thumbnail uint8
        [h'][w'][C], (w', h') = preview_size(W, H, shift): sample (Y, X) is pixel (min(Y S + S / 2, H - 1), min(X S + S / 2, W - 1)), S = 2^shift, of what
        decode_image_tiled returns for the planes with every node at or above 2^levels set to 0."""
        co = np.ascontiguousarray(coefs, np.int32).reshape(-1)
        assert not 0 <= levels <= 9 or co.size == self.n_tiles * self.channels * self.num_cells << levels  # (levels out of range: the library's refusal)
        w, h = preview_size(self.width, self.height, shift)
        out = np.empty((h, w, self.channels), np.uint8)
        _check(load_library().fri_hip_preview_image_tiled(self._h, _p(co), int(levels), int(shift), _p(_q(qmatrix)), _p(out)), "fri_hip_preview_image_tiled", self.ctx)
        return out

    def preview_coded(self, coded, levels, shift, qmatrix=None):
        """fri_hip_preview_image_tiled_coded: the coded planes of a `frit` file (emit.tiled_parse_coded) through the device decoder bounded by `levels` and K14 ->
        (thumbnail uint8 [h'][w'][C], status uint32 [n_tiles C][4]); the thumbnail is preview()'s of emit.tiled_decode_levels's planes. A plane the decoder refuses
        raises FriHipError (-1) with the status as .status. Needs set_stream_order()."""
        planes = self.n_tiles * self.channels
        words, n_words, models, off, vp, wp = _coded_planes(coded, planes)
        w, h = preview_size(self.width, self.height, shift)
        out, status = np.empty((h, w, self.channels), np.uint8), np.zeros((planes, 4), np.uint32)
        rc = load_library().fri_hip_preview_image_tiled_coded(self._h, _p(words), words.shape[1], _p(n_words), _p(models), _p(off), _p(vp), _p(wp), int(levels), int(shift),
                                                              _p(_q(qmatrix)), _p(out), _p(status))
        _check_decode(rc, "fri_hip_preview_image_tiled_coded", self.ctx, status)
        return out, status

    # ---- region decode: only the tiles a rectangle touches -------------------------------------------
    def region_tiles(self, x, y, w, h):
        """fri_hip_plan_tiled_region: (i0, j0, ni, nj), the sub-grid of tiles the region x, y, w, h (image pixels) touches; sub-tile b ni + a is tile
        (j0 + b) nx + (i0 + a). Works on a host-only plan. FriHipError (-1) for an empty region or one that leaves the image."""
        out = np.zeros(4, np.uint32)
        _check(load_library().fri_hip_plan_tiled_region(self._h, x, y, w, h, _p(out)), "fri_hip_plan_tiled_region", self.ctx)
        return tuple(int(v) for v in out)

    def merge_tiles_region_dev(self, d_tiles, x, y, w, h, d_region, stream=0):
        """fri_hip_merge_tiles_region_dev: the sub-grid's tile raster [nj ni][tile_h][tile_w][C] -> the region raster [h][w][C]; only enqueues."""
        _check(load_library().fri_hip_merge_tiles_region_dev(self._h, d_tiles, x, y, w, h, d_region, stream), "fri_hip_merge_tiles_region_dev", self.ctx)

    def decode_region_tiled_dev(self, d_coefs, x, y, w, h, d_region, qmatrix=None, stream=0):
        """fri_hip_decode_region_tiled_dev: d_coefs int32 [nj ni][C][F][512] -> d_region uint8 [h][w][C], device pointers: the inverse kernel over the touched tiles
        into the plan's tile buffer, then the region kernel. Refuses a capturing stream."""
        _check(load_library().fri_hip_decode_region_tiled_dev(self._h, d_coefs, _p(_q(qmatrix)), x, y, w, h, d_region, stream), "fri_hip_decode_region_tiled_dev", self.ctx)

    def decode_region_tiled(self, coefs, x, y, w, h, qmatrix=None):
        """fri_hip_decode_region_tiled: coefs int32 [nj ni][C][F][512] (what emit.tiled_decode_region returns) -> pixels uint8 [h * w * C]: the crop
        [y : y + h, x : x + w] of what decode_image_tiled returns for the same file."""
        _, _, ni, nj = self.region_tiles(x, y, w, h)
        co = np.ascontiguousarray(coefs, np.int32).reshape(-1)
        assert co.size == ni * nj * self.channels * self.num_cells * 512
        out = np.empty(w * h * self.channels, np.uint8)
        _check(load_library().fri_hip_decode_region_tiled(self._h, _p(co), _p(_q(qmatrix)), x, y, w, h, _p(out)), "fri_hip_decode_region_tiled", self.ctx)
        return out

    # ---- several regions per call: the tile list, the region table and K15 ----------------------------
    @staticmethod
    def _regions(regions):
        """regions as the contiguous uint32 [R][4] array the C side reads; a shape or a value it cannot hold is the library's refusal (-1)"""
        try:
            wide = np.asarray(regions, np.int64).reshape(-1, 4)
        except (ValueError, TypeError, OverflowError):
            raise FriHipError(-1, "regions must be rows of (x, y, w, h)", "") from None
        if (wide < 0).any() or (wide > 0xFFFFFFFF).any():
            raise FriHipError(-1, "regions must be rows of (x, y, w, h), each in 32 bits", "")
        return np.ascontiguousarray(wide, np.uint32)

    def _split_regions(self, packed, rg):
        """the packed rasters as a list of [h][w][C] views, region after region"""
        out, at = [], 0
        for _, _, w, h in rg.tolist():
            out.append(packed[at : at + w * h * self.channels].reshape(h, w, self.channels))
            at += w * h * self.channels
        return out

    @staticmethod
    def _packed_bytes(table, n_regions):
        """the packed output's bytes: words 4, 5 of row R of a region table"""
        return int(table[8 * n_regions + 4]) | int(table[8 * n_regions + 5]) << 32

    def _regions_table(self, entry, lead, rg):
        """the size query of fri_hip_plan_tiled[_preview]_regions (`entry`, after the plan its arguments `lead`), then the call -> (list, table)"""
        n = C.c_size_t(0)
        call = getattr(load_library(), entry)
        rc = call(self._h, *lead, rg.shape[0], _p(rg), None, 0, C.addressof(n), None, 0)
        if rc != -3:  # (the size query's answer: the buffers are too small, n is filled)
            _check(rc or -1, entry, self.ctx)
        tiles, table = np.zeros(n.value, np.uint32), np.zeros(8 * (rg.shape[0] + 1) + self.n_tiles, np.uint32)
        _check(call(self._h, *lead, rg.shape[0], _p(rg), _p(tiles), tiles.size, C.addressof(n), _p(table), table.size), entry, self.ctx)
        return tiles, table

    def _regions_coded(self, entry, coded, rg, tiles, table, tail):
        """a coded regions call `entry` (after the coded planes its arguments `tail`, then the output and the status) -> (a list of [h][w][C] arrays, status); a
        refusal carries the file-grid index of the first refused plane's tile as .tile"""
        planes = tiles.size * self.channels
        words, n_words, models, off, vp, wp = _coded_planes(coded, planes)
        out = np.empty(self._packed_bytes(table, rg.shape[0]), np.uint8)
        status = np.zeros((planes, 4), np.uint32)
        rc = getattr(load_library(), entry)(self._h, rg.shape[0], _p(rg), _p(words), words.shape[1], _p(n_words), _p(models), _p(off), _p(vp), _p(wp), *tail, _p(out), _p(status))
        try:
            _check_decode(rc, entry, self.ctx, status)
        except FriHipError as e:
            bad = np.flatnonzero(status[:, 0])
            e.tile = int(tiles[bad[0] // self.channels]) if bad.size else None
            raise
        return self._split_regions(out, rg), status

    def regions(self, regions):
        """fri_hip_plan_tiled_regions: (list uint32 [T], table uint32 [8 (R + 1) + nx ny]) of `regions` [(x, y, w, h), ...] - the strictly ascending file-grid
        indices of the tiles at least one region touches, and the region table K15 reads (include/fri_hip.h, "Several regions"; its row R holds the packed
        output's bytes in words 4, 5 and n_groups in word 6). Works on a host-only plan. FriHipError (-1) for no regions, more than 65535, a region that is
        empty or leaves the image, n_groups >= 2^31. The plan remembers the last table it wrote: merge_tiles_regions_dev takes that one."""
        return self._regions_table("fri_hip_plan_tiled_regions", (), self._regions(regions))

    def merge_tiles_regions_dev(self, d_tiles, n_list, n_regions, d_table, d_out, stream=0):
        """fri_hip_merge_tiles_regions_dev (K15 alone), device pointers as ints: the tile-list raster [T][tile_h][tile_w][C] -> the packed region rasters. d_table
        must be, in device memory, the table regions() LAST returned on this plan, n_list and n_regions its T and R. Only enqueues; capturable."""
        _check(load_library().fri_hip_merge_tiles_regions_dev(self._h, d_tiles, int(n_list), int(n_regions), d_table, d_out, stream), "fri_hip_merge_tiles_regions_dev", self.ctx)

    def decode_regions_tiled_dev(self, d_coefs, regions, d_out, qmatrix=None, stream=0):
        """fri_hip_decode_regions_tiled_dev: d_coefs int32 [T][C][F][512] in list order -> d_out, the packed region rasters, device pointers: the inverse kernel
        over the listed tiles into the plan's tile buffer, then K15. `regions` is host memory. Refuses a capturing stream."""
        rg = self._regions(regions)
        _check(load_library().fri_hip_decode_regions_tiled_dev(self._h, d_coefs, _p(_q(qmatrix)), rg.shape[0], _p(rg), d_out, stream), "fri_hip_decode_regions_tiled_dev", self.ctx)

    def decode_regions_tiled(self, coefs, regions, qmatrix=None):
        """fri_hip_decode_regions_tiled: coefs int32 [T][C][F][512] (what emit.tiled_decode_tiles returns for regions()'s list) -> a list of uint8 [h][w][C]
        arrays, one per region: each the crop [y : y + h, x : x + w] of what decode_image_tiled returns for the same file."""
        rg = self._regions(regions)
        tiles, table = self.regions(rg)
        co = np.ascontiguousarray(coefs, np.int32).reshape(-1)
        assert co.size == tiles.size * self.channels * self.num_cells * 512
        out = np.empty(self._packed_bytes(table, rg.shape[0]), np.uint8)
        _check(load_library().fri_hip_decode_regions_tiled(self._h, _p(co), _p(_q(qmatrix)), rg.shape[0], _p(rg), _p(out)), "fri_hip_decode_regions_tiled", self.ctx)
        return self._split_regions(out, rg)

    def decode_regions_coded(self, coded, regions, qmatrix=None):
        """fri_hip_decode_regions_tiled_coded: the coded planes of regions()'s tile list - what emit.tiled_parse_coded_tiles returns, with or without its TiledInfo -
        through the device decoder (K13) over the T C planes, the inverse kernel and K15 -> (a list of uint8 [h][w][C] arrays, status uint32 [T C][4]); the arrays
        are decode_regions_tiled's of emit.tiled_decode_tiles's planes. A plane the decoder refuses raises FriHipError (-1) with the status as .status and the
        file-grid index of the first refused plane's tile as .tile. Needs set_stream_order()."""
        rg = self._regions(regions)
        tiles, table = self.regions(rg)
        return self._regions_coded("fri_hip_decode_regions_tiled_coded", coded, rg, tiles, table, (_p(_q(qmatrix)),))

    # ---- preview of regions: several rectangles of the thumbnail in one call (K17) ---------------------
    def preview_regions_table(self, shift, regions):
        """fri_hip_plan_tiled_preview_regions: (list uint32 [T], table uint32 [8 (R + 1) + nx ny]) of `regions` [(X, Y, w, h), ...] in the coordinates of the
        thumbnail at `shift` - the tile list of their source rectangles and the preview-region table K17 reads (include/fri_hip.h, "Preview of regions"; its row R
        holds the packed output's bytes in words 4, 5 and n_groups in word 6). Works on a host-only plan. FriHipError (-1) for shift > 4, no regions, more than
        65535, a region that is empty or leaves the thumbnail, n_groups >= 2^31. The plan remembers the last such table: preview_tiles_regions_dev takes that one."""
        return self._regions_table("fri_hip_plan_tiled_preview_regions", (int(shift),), self._regions(regions))

    def preview_tiles_regions_dev(self, d_coefs, coef_stride, node_stride, levels, shift, n_list, n_regions, d_table, d_out, qmatrix=None, stream=0):
        """fri_hip_preview_tiles_regions_dev (K17 alone), device pointers as ints: the listed tiles' planes [T][C] coef_stride elements apart, node h of cell k at
        k * node_stride + h (node_stride 512 or 2^levels) -> the packed region rasters, any alignment. d_table must be, in device memory, the table
        preview_regions_table() LAST returned on this plan, n_list, n_regions and shift its T, R and m. Only enqueues; capturable."""
        _check(load_library().fri_hip_preview_tiles_regions_dev(self._h, d_coefs, coef_stride, node_stride, int(levels), int(shift), _p(_q(qmatrix)), int(n_list), int(n_regions),
                                                                d_table, d_out, stream), "fri_hip_preview_tiles_regions_dev", self.ctx)

    def preview_regions(self, coefs, levels, shift, regions, qmatrix=None):
        """fri_hip_preview_regions_tiled: the compact planes int32 [T][C][F][2^levels] (what emit.tiled_decode_tiles_levels returns for preview_regions_table()'s list)
        -> a list of uint8 [h][w][C] arrays, one per region: each the crop [Y : Y + h, X : X + w] of what preview() returns for the same file, levels and shift."""
        rg = self._regions(regions)
        tiles, table = self.preview_regions_table(shift, rg)
        co = np.ascontiguousarray(coefs, np.int32).reshape(-1)
        assert not 0 <= levels <= 9 or co.size == tiles.size * self.channels * self.num_cells << levels  # (levels out of range: the library's refusal)
        out = np.empty(self._packed_bytes(table, rg.shape[0]), np.uint8)
        _check(load_library().fri_hip_preview_regions_tiled(self._h, _p(co), int(levels), int(shift), _p(_q(qmatrix)), rg.shape[0], _p(rg), _p(out)),
               "fri_hip_preview_regions_tiled", self.ctx)
        return self._split_regions(out, rg)

    def preview_regions_coded(self, coded, levels, shift, regions, qmatrix=None):
        """fri_hip_preview_regions_tiled_coded: the coded planes of preview_regions_table()'s tile list - what emit.tiled_parse_coded_tiles returns, with or without
        its TiledInfo - through the device decoder bounded by `levels` over the T C planes and K17 -> (a list of uint8 [h][w][C] arrays, status uint32 [T C][4]); the
        arrays are preview_regions()'s of emit.tiled_decode_tiles_levels's planes. A plane the decoder refuses raises FriHipError (-1) with the status as .status
        and the file-grid index of the first refused plane's tile as .tile. Needs set_stream_order()."""
        rg = self._regions(regions)
        tiles, table = self.preview_regions_table(shift, rg)
        return self._regions_coded("fri_hip_preview_regions_tiled_coded", coded, rg, tiles, table, (int(levels), int(shift), _p(_q(qmatrix))))

    # ---- region update: only the tiles a rectangle touches are split and coded ------------------------
    def region_cover(self, x, y, w, h):
        """fri_hip_plan_tiled_region_cover: (cx, cy, cw, ch), the covered rectangle of the region x, y, w, h - the in-image pixels of the tiles it touches, the
        only pixels a region encode reads. Works on a host-only plan. FriHipError (-1) as region_tiles."""
        out = np.zeros(4, np.uint32)
        _check(load_library().fri_hip_plan_tiled_region_cover(self._h, x, y, w, h, _p(out)), "fri_hip_plan_tiled_region_cover", self.ctx)
        return tuple(int(v) for v in out)

    def split_tiles_region_dev(self, d_src, src_pitch, src_x, src_y, src_w, src_h, x, y, w, h, d_tiles, stream=0):
        """fri_hip_split_tiles_region_dev: a pitched rectangle of the image (d_src points at image pixel (src_y, src_x); it must contain the covered rectangle) ->
        the sub-grid's tile raster [nj ni][tile_h][tile_w][C], the sub-grid's rows of split_tiles_dev; only enqueues."""
        _check(load_library().fri_hip_split_tiles_region_dev(self._h, d_src, src_pitch, src_x, src_y, src_w, src_h, x, y, w, h, d_tiles, stream),
               "fri_hip_split_tiles_region_dev", self.ctx)

    def encode_symbols_region_tiled_dev(self, d_src, src_pitch, src_x, src_y, src_w, src_h, x, y, w, h, d_params, d_symbols, d_hist, d_oob, d_fit_out_of_range=None,
                                        qmatrix=None, fit=True, stream=0):
        """fri_hip_encode_symbols_region_tiled_dev: the region split and one direct stream chain over the touched tiles, everything on the device, the outputs in
        the sub-grid's order with the layouts of encode_symbols_tiled_dev. Needs set_stream_order(); refuses a capturing stream."""
        _check(load_library().fri_hip_encode_symbols_region_tiled_dev(self._h, d_src, src_pitch, src_x, src_y, src_w, src_h, x, y, w, h, _p(_q(qmatrix)), int(bool(fit)),
                                                                     d_params, d_symbols, d_hist, d_oob, d_fit_out_of_range, stream),
               "fri_hip_encode_symbols_region_tiled_dev", self.ctx)

    def encode_region_tiled_symbols(self, pixels, x, y, w, h, qmatrix=None):
        """fri_hip_encode_region_tiled_symbols: pixels is the whole raster [H][W][C], of which only the covered rectangle is copied to the device - (symbols uint16
        [nj ni][C][num_some], value_params, width_params [nj ni][C][3][6], hist [nj ni][C][10][1024], oob [nj ni][C]) in the sub-grid's order: what
        emit.tiled_update_from_streams takes; the fit is on. Needs set_stream_order()."""
        px = np.ascontiguousarray(pixels, np.uint8).reshape(-1)
        assert px.size == self.pixel_bytes
        _, _, ni, nj = self.region_tiles(x, y, w, h)
        n, c = ni * nj, self.channels
        vp, wp = np.zeros((n, c, 3, 6), np.float32), np.zeros((n, c, 3, 6), np.float32)
        sym = np.empty((n, c, self.num_some), np.uint16)
        hist = np.empty((n, c, 10, 1024), np.uint32)
        oob = np.zeros((n, c), np.uint64)
        _check(load_library().fri_hip_encode_region_tiled_symbols(self._h, _p(px), x, y, w, h, _p(_q(qmatrix)), _p(vp), _p(wp), _p(sym), _p(hist), _p(oob)),
               "fri_hip_encode_region_tiled_symbols", self.ctx)
        return sym, vp, wp, hist, oob

    # ---- the measure, the size estimate and the searches over tiles ----------------------------------
    def measure_distortion_tiled_dev(self, d_tiles, d_reference_raster, d_out, stream=0):
        """fri_hip_measure_distortion_tiled_dev: the tile raster's in-image pixels against a raster [H][W][C]; d_out (uint64 [2 C + 1], device) = per channel c the
        sum of squared differences at 2 c and the largest absolute difference at 2 c + 1, the pixels counted (W H) at 2 C. Only enqueues."""
        _check(load_library().fri_hip_measure_distortion_tiled_dev(self._h, d_tiles, d_reference_raster, d_out, stream), "fri_hip_measure_distortion_tiled_dev", self.ctx)

    def estimate_size_tiled_dev(self, d_hist, d_oob, d_file_bytes, d_tile_bytes, d_models=None, stream=0):
        """fri_hip_estimate_size_tiled_dev: d_hist uint32 [n_tiles][C][10][1024], d_oob uint64 [n_tiles][C] or None -> d_file_bytes uint64 [1], d_tile_bytes uint64
        [n_tiles] and, if given, d_models uint32 [n_tiles][C][10][4]; device pointers. Only enqueues."""
        _check(load_library().fri_hip_estimate_size_tiled_dev(self._h, d_hist, d_oob or None, d_file_bytes, d_tile_bytes, d_models or None, stream),
               "fri_hip_estimate_size_tiled_dev", self.ctx)

    def estimate_size_tiled(self, hist, oob=None):
        """fri_hip_estimate_size_tiled: hist [n_tiles][C][10][1024] (oob [n_tiles][C] or None), host arrays -> (file bytes, tile bytes uint64 [n_tiles]): the
        estimated size of the `frit` file and of its payloads (include/fri_hip.h gives the formula); UINT64_MAX where the emitter would refuse a tile."""
        h = np.ascontiguousarray(hist, np.uint32)
        assert h.size == self.n_tiles * self.channels * 10 * 1024
        o = None if oob is None else np.ascontiguousarray(oob, np.uint64)
        assert o is None or o.size == self.n_tiles * self.channels
        total, tiles = C.c_uint64(0), np.zeros(self.n_tiles, np.uint64)
        _check(load_library().fri_hip_estimate_size_tiled(self._h, _p(h), None if o is None else _p(o), C.byref(total), _p(tiles)), "fri_hip_estimate_size_tiled", self.ctx)
        return total.value, tiles

    def search_quality(self, pixels, target_db, stream=0):
        """fri_hip_search_quality_tiled[_dev] (pixels: a host array or a device pointer): (quality, PSNR in dB of the tiled round trip); 100 = code losslessly."""
        return _search(self, "fri_hip_search_quality_tiled", pixels, float(target_db), C.c_double, stream)

    def search_quality_ssim(self, pixels, target, stream=0):
        """fri_hip_search_quality_ssim_tiled[_dev]: (quality, SSIM of the tiled round trip); 100 = code losslessly."""
        return _search(self, "fri_hip_search_quality_ssim_tiled", pixels, float(target), C.c_double, stream)

    def search_quality_for_size(self, pixels, max_bytes, stream=0):
        """fri_hip_search_quality_for_size_tiled[_dev]: (quality, estimated bytes of the `frit` file); FriHipError with code -7 when nothing fits. Needs
        set_stream_order()."""
        return _search(self, "fri_hip_search_quality_for_size_tiled", pixels, int(max_bytes), C.c_uint64, stream)


class PlanTiled420:
    """fri_hip_plan_tiled420: an image as a batch of independently coded 4:2:0 tiles (include/fri_hip.h, "Tiled 4:2:0 coding", has the format). Owns two ordinary
    C = 1 plans, .luma (tile_w x tile_h) and .chroma (cw x ch) - Plan views that do not own their handle and die with this object. Every per-plane array is in
    plane order: with n tiles, plane(t, Y) = t, plane(t, Cb) = n + 2 t, plane(t, Cr) = n + 2 t + 1. ctx=None gives a host-only plan (getters only). flags:
    TILED_ALLOW_HOLES accepts a tile shape at which a lattice does not own every pixel. Calls on one PlanTiled420 must be ordered on one stream: they share the
    plan's staging buffers."""

    def __init__(self, ctx, width, height, tile_w, tile_h, flags=0):
        self._h = None
        self.ctx = ctx
        self.width, self.height = width, height
        h = C.c_void_p()
        L = load_library()
        _check(L.fri_hip_plan_tiled420_create(ctx._h if ctx else None, width, height, tile_w, tile_h, flags, C.byref(h)), "fri_hip_plan_tiled420_create", ctx)
        self._h = h
        self.cw, self.ch = (tile_w + 1) // 2, (tile_h + 1) // 2
        self.luma = Plan(ctx, tile_w, tile_h, 1, _handle=L.fri_hip_plan_tiled420_luma(h))
        self.chroma = Plan(ctx, self.cw, self.ch, 1, _handle=L.fri_hip_plan_tiled420_chroma(h))
        grid = np.zeros(4, np.uint32)
        _check(L.fri_hip_plan_tiled420_grid(h, _p(grid)), "fri_hip_plan_tiled420_grid", ctx)
        self.nx, self.ny, self.tile_w, self.tile_h = (int(v) for v in grid)
        self.n_tiles = self.nx * self.ny
        self.pixel_bytes = width * height * 3
        self.y_tile_bytes = self.n_tiles * tile_w * tile_h      # y_tiles [n][tile_h][tile_w]
        self.c_tile_bytes = self.n_tiles * 2 * self.cw * self.ch  # c_tiles [n][2][ch][cw]
        self.n_luma, self.n_chroma = self.luma.num_some, self.chroma.num_some  # symbols of a tile's luma plane and of one of its chroma planes
        self.num_symbols = self.n_tiles * (self.n_luma + 2 * self.n_chroma)
        self.tile_coef_count = (self.luma.num_cells + 2 * self.chroma.num_cells) * 512
        self.coef_count = self.n_tiles * self.tile_coef_count

    def close(self):
        if self._h:
            self.luma.close()
            self.chroma.close()
            load_library().fri_hip_plan_tiled420_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream_order(self):
        """fri_hip_plan_set_stream_order on both inner plans (the encodes need it)."""
        self.luma.set_stream_order()
        self.chroma.set_stream_order()

    def region_tiles(self, x, y, w, h):
        """fri_hip_plan_tiled420_region: (i0, j0, ni, nj), the sub-grid of tiles the region touches. Works on a host-only plan. FriHipError (-1) for an empty
        region or one that leaves the image."""
        out = np.zeros(4, np.uint32)
        _check(load_library().fri_hip_plan_tiled420_region(self._h, x, y, w, h, _p(out)), "fri_hip_plan_tiled420_region", self.ctx)
        return tuple(int(v) for v in out)

    def buffer_tiles(self):
        """fri_hip_plan_tiled420_buffer_tiles: the tiles the plan's (luma, chroma) tile buffers hold room for at the moment."""
        out = np.zeros(2, np.uint64)
        _check(load_library().fri_hip_plan_tiled420_buffer_tiles(self._h, _p(out)), "fri_hip_plan_tiled420_buffer_tiles", self.ctx)
        return int(out[0]), int(out[1])

    # ---- device-pointer entry points (pointers are ints) --------------------------------------------
    def split_tiles420_dev(self, d_rgb, d_y_tiles, d_c_tiles, stream=0):
        """fri_hip_split_tiles420_dev: [H][W][3] -> y_tiles [n][tile_h][tile_w] and c_tiles [n][2][ch][cw] in one pass; only enqueues."""
        _check(load_library().fri_hip_split_tiles420_dev(self._h, d_rgb, d_y_tiles, d_c_tiles, stream), "fri_hip_split_tiles420_dev", self.ctx)

    def merge_tiles420_dev(self, d_y_tiles, d_c_tiles, d_rgb, stream=0):
        """fri_hip_merge_tiles420_dev: the tiles' planes -> [H][W][3], every pixel upsampled within its own tile; only enqueues."""
        _check(load_library().fri_hip_merge_tiles420_dev(self._h, d_y_tiles, d_c_tiles, d_rgb, stream), "fri_hip_merge_tiles420_dev", self.ctx)

    def merge_tiles420_region_dev(self, d_y_tiles, d_c_tiles, x, y, w, h, d_region, stream=0):
        """fri_hip_merge_tiles420_region_dev: the sub-grid's planes -> the region raster [h][w][3]; only enqueues."""
        _check(load_library().fri_hip_merge_tiles420_region_dev(self._h, d_y_tiles, d_c_tiles, x, y, w, h, d_region, stream), "fri_hip_merge_tiles420_region_dev", self.ctx)

    def encode_symbols_tiled420_dev(self, d_rgb, quality, d_params, d_symbols, d_hist, d_oob, d_fit_out_of_range=None, fit=True, stream=0):
        """fri_hip_encode_symbols_tiled420_dev: the split and the direct stream chain on both inner plans, everything on the device and in plane order: d_params
        float32 [3 n][2][3][6], d_symbols uint16 [n][n_luma] then [n][2][n_chroma], d_hist uint32 [3 n][10][1024], d_oob uint64 [3 n], d_fit_out_of_range uint64
        [3 n] or None. Needs set_stream_order()."""
        _check(load_library().fri_hip_encode_symbols_tiled420_dev(self._h, d_rgb, int(quality), int(bool(fit)), d_params, d_symbols, d_hist, d_oob, d_fit_out_of_range, stream),
               "fri_hip_encode_symbols_tiled420_dev", self.ctx)

    def decode_region_tiled420_dev(self, d_coefs, quality, x, y, w, h, d_region, stream=0):
        """fri_hip_decode_region_tiled420_dev: d_coefs int32, the sub-grid's planes in plane order -> d_region uint8 [h][w][3], device pointers. Refuses a
        capturing stream."""
        _check(load_library().fri_hip_decode_region_tiled420_dev(self._h, d_coefs, int(quality), x, y, w, h, d_region, stream), "fri_hip_decode_region_tiled420_dev", self.ctx)

    # ---- host-pointer entry points ----------------------------------------------------------------
    def encode_image_tiled420_symbols(self, pixels, quality):
        """fri_hip_encode_image_tiled420_symbols: (symbols uint16 flat = [n][n_luma] then [n][2][n_chroma], value_params [3 n][3][6], width_params [3 n][3][6],
        hist [3 n][10][1024], oob [3 n]), all in plane order - what emit.tiled_encode_from_streams420 takes; the fit is on. Needs set_stream_order()."""
        px = np.ascontiguousarray(pixels, np.uint8).reshape(-1)
        assert px.size == self.pixel_bytes
        planes = 3 * self.n_tiles
        vp, wp = np.zeros((planes, 3, 6), np.float32), np.zeros((planes, 3, 6), np.float32)
        sym = np.empty(self.num_symbols, np.uint16)
        hist = np.empty((planes, 10, 1024), np.uint32)
        oob = np.zeros(planes, np.uint64)
        _check(load_library().fri_hip_encode_image_tiled420_symbols(self._h, _p(px), int(quality), _p(vp), _p(wp), _p(sym), _p(hist), _p(oob)),
               "fri_hip_encode_image_tiled420_symbols", self.ctx)
        return sym, vp, wp, hist, oob

    def decode_image_tiled420(self, coefs, quality):
        """fri_hip_decode_image_tiled420: coefs int32 in plane order (what emit.tiled_decode returns for a tiled 4:2:0 file) -> pixels uint8 [H * W * 3]."""
        co = np.ascontiguousarray(coefs, np.int32).reshape(-1)
        assert co.size == self.coef_count
        out = np.empty(self.pixel_bytes, np.uint8)
        _check(load_library().fri_hip_decode_image_tiled420(self._h, _p(co), int(quality), _p(out)), "fri_hip_decode_image_tiled420", self.ctx)
        return out

    def decode_coded(self, coded, quality):
        """fri_hip_decode_image_tiled420_coded: the coded planes of a tiled 4:2:0 file in plane order - what emit.tiled_parse_coded returns, with or without its
        TiledInfo - through the device decoder (K13) on both lattices, the inverse kernels and the merge -> (pixels uint8 [H * W * 3], status uint32 [3 n][4]).
        A plane the decoder refuses raises FriHipError (-1) with the status as .status. Needs set_stream_order()."""
        planes = 3 * self.n_tiles
        words, n_words, models, off, vp, wp = _coded_planes(coded, planes)
        out, status = np.empty(self.pixel_bytes, np.uint8), np.zeros((planes, 4), np.uint32)
        rc = load_library().fri_hip_decode_image_tiled420_coded(self._h, _p(words), words.shape[1], _p(n_words), _p(models), _p(off), _p(vp), _p(wp), int(quality), _p(out),
                                                                _p(status))
        _check_decode(rc, "fri_hip_decode_image_tiled420_coded", self.ctx, status)
        return out, status

    def decode_region_tiled420(self, coefs, quality, x, y, w, h):
        """fri_hip_decode_region_tiled420: coefs int32, the sub-grid's planes in plane order (what emit.tiled_decode_region returns) -> pixels uint8 [h * w * 3]:
        the crop [y : y + h, x : x + w] of what decode_image_tiled420 returns for the same file."""
        _, _, ni, nj = self.region_tiles(x, y, w, h)
        co = np.ascontiguousarray(coefs, np.int32).reshape(-1)
        assert co.size == ni * nj * self.tile_coef_count
        out = np.empty(w * h * 3, np.uint8)
        _check(load_library().fri_hip_decode_region_tiled420(self._h, _p(co), int(quality), x, y, w, h, _p(out)), "fri_hip_decode_region_tiled420", self.ctx)
        return out

    # ---- several regions per call: the tile list, the 4:2:0 region table and K18 -----------------------
    channels = 3  # of every raster this plan decodes (what PlanTiled's region helpers read)

    def regions(self, regions):
        """fri_hip_plan_tiled420_regions: (list uint32 [T], table uint32 [8 (R + 1) + nx ny]) of `regions` [(x, y, w, h), ...] - the strictly ascending file-grid
        indices of the tiles at least one region touches, and the 4:2:0 region table K18 reads (include/fri_hip.h, "Several regions of tiled 4:2:0 files": strips
        of 16 pixels; its row R holds the packed output's bytes in words 4, 5 and n_groups in word 6). Works on a host-only plan. FriHipError (-1) for no regions,
        more than 65535, a region that is empty or leaves the image, n_groups >= 2^31. The plan remembers the last table it wrote: merge_tiles420_regions_dev
        takes that one."""
        return PlanTiled._regions_table(self, "fri_hip_plan_tiled420_regions", (), PlanTiled._regions(regions))

    def merge_tiles420_regions_dev(self, d_y_tiles, d_c_tiles, n_list, n_regions, d_table, d_out, stream=0):
        """fri_hip_merge_tiles420_regions_dev (K18 alone), device pointers as ints: the tile-list planes y_tiles [T][tile_h][tile_w] and c_tiles [T][2][ch][cw] ->
        the packed region rasters [h][w][3]. d_table must be, in device memory, the table regions() LAST returned on this plan, n_list and n_regions its T and R.
        Only enqueues; capturable."""
        _check(load_library().fri_hip_merge_tiles420_regions_dev(self._h, d_y_tiles, d_c_tiles, int(n_list), int(n_regions), d_table, d_out, stream),
               "fri_hip_merge_tiles420_regions_dev", self.ctx)

    def decode_regions_tiled420_dev(self, d_coefs, quality, regions, d_out, stream=0):
        """fri_hip_decode_regions_tiled420_dev: d_coefs int32, the listed tiles' planes in plane order with n = T -> d_out, the packed region rasters, device
        pointers: the inverse kernels over the listed tiles into the plan's tile buffers, then K18. `regions` is host memory. Refuses a capturing stream."""
        rg = PlanTiled._regions(regions)
        _check(load_library().fri_hip_decode_regions_tiled420_dev(self._h, d_coefs, int(quality), rg.shape[0], _p(rg), d_out, stream), "fri_hip_decode_regions_tiled420_dev",
               self.ctx)

    def decode_regions_tiled420(self, coefs, quality, regions):
        """fri_hip_decode_regions_tiled420: coefs int32 in plane order with n = T (what emit.tiled_decode_tiles returns for regions()'s list) -> a list of uint8
        [h][w][3] arrays, one per region: each the crop [y : y + h, x : x + w] of what decode_image_tiled420 returns for the same file."""
        rg = PlanTiled._regions(regions)
        tiles, table = self.regions(rg)
        co = np.ascontiguousarray(coefs, np.int32).reshape(-1)
        assert co.size == tiles.size * self.tile_coef_count
        out = np.empty(PlanTiled._packed_bytes(table, rg.shape[0]), np.uint8)
        _check(load_library().fri_hip_decode_regions_tiled420(self._h, _p(co), int(quality), rg.shape[0], _p(rg), _p(out)), "fri_hip_decode_regions_tiled420", self.ctx)
        return PlanTiled._split_regions(self, out, rg)

    def decode_regions_coded(self, coded, quality, regions):
        """fri_hip_decode_regions_tiled420_coded: the coded planes of regions()'s tile list in plane order with n = T - what emit.tiled_parse_coded_tiles returns,
        with or without its TiledInfo - through the device decoder (K13) on both lattices, the inverse kernels and K18 -> (a list of uint8 [h][w][3] arrays, status
        uint32 [3 T][4]); the arrays are decode_regions_tiled420's of emit.tiled_decode_tiles's planes. A plane the decoder refuses raises FriHipError (-1) with
        the status as .status and the file-grid index of the first refused plane's tile as .tile. Needs set_stream_order()."""
        rg = PlanTiled._regions(regions)
        tiles, table = self.regions(rg)
        n, planes = tiles.size, 3 * tiles.size
        words, n_words, models, off, vp, wp = _coded_planes(coded, planes)
        out = np.empty(PlanTiled._packed_bytes(table, rg.shape[0]), np.uint8)
        status = np.zeros((planes, 4), np.uint32)
        rc = load_library().fri_hip_decode_regions_tiled420_coded(self._h, rg.shape[0], _p(rg), _p(words), words.shape[1], _p(n_words), _p(models), _p(off), _p(vp), _p(wp),
                                                                  int(quality), _p(out), _p(status))
        try:
            _check_decode(rc, "fri_hip_decode_regions_tiled420_coded", self.ctx, status)
        except FriHipError as e:
            bad = np.flatnonzero(status[:, 0])
            e.tile = int(tiles[bad[0] if bad[0] < n else (bad[0] - n) // 2]) if bad.size else None
            raise
        return PlanTiled._split_regions(self, out, rg), status

    def encode_image_tiled420_coded(self, pixels, quality, word_stride=None):
        """fri_hip_encode_image_tiled420_coded: the tiled 4:2:0 chain with the fit, then the device rANS coder over the luma batch and the chroma batch - (words
        uint32 [3 n][word_stride], n_words uint32 [3 n], models uint32 [3 n][10][4], off_values uint16 [3 n][10][1024], status uint32 [3 n][4], value_params,
        width_params [3 n][3][6]), all in plane order: what emit.tiled_encode_from_coded420 takes. word_stride: words per plane of the returned array (default
        max(n_luma, n_chroma) + 20, which always suffices). Needs set_stream_order()."""
        px = np.ascontiguousarray(pixels, np.uint8).reshape(-1)
        assert px.size == self.pixel_bytes
        planes = 3 * self.n_tiles
        stride = max(self.n_luma, self.n_chroma) + 20 if word_stride is None else int(word_stride)
        vp, wp = np.zeros((planes, 3, 6), np.float32), np.zeros((planes, 3, 6), np.float32)
        words = np.zeros((planes, stride), np.uint32)
        n_words, models = np.zeros(planes, np.uint32), np.zeros((planes, 10, 4), np.uint32)
        off, status = np.zeros((planes, 10, 1024), np.uint16), np.zeros((planes, 4), np.uint32)
        _check(load_library().fri_hip_encode_image_tiled420_coded(self._h, _p(px), int(quality), _p(vp), _p(wp), _p(words), stride, _p(n_words), _p(models), _p(off),
                                                                 _p(status)), "fri_hip_encode_image_tiled420_coded", self.ctx)
        return words, n_words, models, off, status, vp, wp

    # ---- the measure, the size estimate and the searches over subsampled tiles ------------------------
    def measure_distortion_tiled420_dev(self, d_y_tiles, d_c_tiles, d_reference_rgb, d_out, stream=0):
        """fri_hip_measure_distortion_tiled420_dev: the merge of the tiles' planes against a raster [H][W][3] with nothing stored; d_out (uint64 [7], device) = per
        channel c (R, G, B) the sum of squared differences at 2 c and the largest absolute difference at 2 c + 1, the pixels counted (W H) at 6. Only enqueues."""
        _check(load_library().fri_hip_measure_distortion_tiled420_dev(self._h, d_y_tiles, d_c_tiles, d_reference_rgb, d_out, stream),
               "fri_hip_measure_distortion_tiled420_dev", self.ctx)

    def estimate_size_tiled420_dev(self, d_hist, d_oob, d_file_bytes, d_tile_bytes, d_models=None, stream=0):
        """fri_hip_estimate_size_tiled420_dev: d_hist uint32 [3 n][10][1024], d_oob uint64 [3 n] or None, in plane order -> d_file_bytes uint64 [1], d_tile_bytes
        uint64 [n] and, if given, d_models uint32 [3 n][10][4]; device pointers. Only enqueues."""
        _check(load_library().fri_hip_estimate_size_tiled420_dev(self._h, d_hist, d_oob or None, d_file_bytes, d_tile_bytes, d_models or None, stream),
               "fri_hip_estimate_size_tiled420_dev", self.ctx)

    def estimate_size_tiled420(self, hist, oob=None):
        """fri_hip_estimate_size_tiled420: hist [3 n][10][1024] (oob [3 n] or None) in plane order, host arrays -> (file bytes, tile bytes uint64 [n]): the
        estimated size of the tiled 4:2:0 `frit` file and of its payloads; UINT64_MAX where the emitter would refuse a tile."""
        h = np.ascontiguousarray(hist, np.uint32)
        assert h.size == 3 * self.n_tiles * 10 * 1024
        o = None if oob is None else np.ascontiguousarray(oob, np.uint64)
        assert o is None or o.size == 3 * self.n_tiles
        total, tiles = C.c_uint64(0), np.zeros(self.n_tiles, np.uint64)
        _check(load_library().fri_hip_estimate_size_tiled420(self._h, _p(h), None if o is None else _p(o), C.byref(total), _p(tiles)), "fri_hip_estimate_size_tiled420",
               self.ctx)
        return total.value, tiles

    def search_quality(self, pixels, target_db, stream=0):
        """fri_hip_search_quality_tiled420[_dev] (pixels: a host array or a device pointer): (quality, PSNR in dB of the tiled 4:2:0 round trip); 100 = no 4:2:0
        quality reaches the target."""
        return _search(self, "fri_hip_search_quality_tiled420", pixels, float(target_db), C.c_double, stream)

    def search_quality_ssim(self, pixels, target, stream=0):
        """fri_hip_search_quality_ssim_tiled420[_dev]: (quality, SSIM of the tiled 4:2:0 round trip); 100 = no 4:2:0 quality reaches the target."""
        return _search(self, "fri_hip_search_quality_ssim_tiled420", pixels, float(target), C.c_double, stream)

    def search_quality_for_size(self, pixels, max_bytes, stream=0):
        """fri_hip_search_quality_for_size_tiled420[_dev]: (quality, estimated bytes of the `frit` file); FriHipError with code -7 when nothing fits. Needs
        set_stream_order()."""
        return _search(self, "fri_hip_search_quality_for_size_tiled420", pixels, int(max_bytes), C.c_uint64, stream)


class PlanTiledRgba:
    """fri_hip_plan_tiled_rgba: an RGBA image as a batch of independently coded RGBA tiles (include/fri_hip.h, "Tiled RGBA coding", has the format). Owns two
    ordinary plans of the tile's shape on one lattice, .colour (C = 3: set the colour transform and the dequantiser of a decode here) and .alpha (C = 1) - Plan
    views that do not own their handle and die with this object. Every per-plane array is in plane order: with n tiles, plane(t, c) = 3 t + c for the colour
    channels and plane(t, A) = 3 n + t. ctx=None gives a host-only plan (getters only). flags: TILED_ALLOW_HOLES accepts a tile shape whose lattice does not own
    every pixel. Calls on one PlanTiledRgba must be ordered on one stream: they share the plan's staging buffers."""

    def __init__(self, ctx, width, height, tile_w, tile_h, flags=0):
        self._h = None
        self.ctx = ctx
        self.width, self.height = width, height
        h = C.c_void_p()
        L = load_library()
        _check(L.fri_hip_plan_tiled_rgba_create(ctx._h if ctx else None, width, height, tile_w, tile_h, flags, C.byref(h)), "fri_hip_plan_tiled_rgba_create", ctx)
        self._h = h
        self.colour = Plan(ctx, tile_w, tile_h, 3, _handle=L.fri_hip_plan_tiled_rgba_colour(h))
        self.alpha = Plan(ctx, tile_w, tile_h, 1, _handle=L.fri_hip_plan_tiled_rgba_alpha(h))
        grid = np.zeros(4, np.uint32)
        _check(L.fri_hip_plan_tiled_rgba_grid(h, _p(grid)), "fri_hip_plan_tiled_rgba_grid", ctx)
        self.nx, self.ny, self.tile_w, self.tile_h = (int(v) for v in grid)
        self.n_tiles = self.nx * self.ny
        self.pixel_bytes = width * height * 4
        self.colour_tile_bytes = self.n_tiles * tile_w * tile_h * 3  # colour_tiles [n][tile_h][tile_w][3]
        self.alpha_tile_bytes = self.n_tiles * tile_w * tile_h       # alpha_tiles [n][tile_h][tile_w]
        self.num_cells = self.colour.num_cells
        self.num_some = self.colour.num_some  # symbols per plane, the same for all four channels of a tile
        self.num_symbols = 4 * self.n_tiles * self.num_some
        self.tile_coef_count = 4 * self.num_cells * 512
        self.coef_count = self.n_tiles * self.tile_coef_count

    def close(self):
        if self._h:
            self.colour.close()
            self.alpha.close()
            load_library().fri_hip_plan_tiled_rgba_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream_order(self):
        """fri_hip_plan_set_stream_order on both inner plans (the encodes need it)."""
        self.colour.set_stream_order()
        self.alpha.set_stream_order()

    def grid(self):
        """fri_hip_plan_tiled_rgba_grid: (nx, ny, tile_w, tile_h). Works on a host-only plan."""
        out = np.zeros(4, np.uint32)
        _check(load_library().fri_hip_plan_tiled_rgba_grid(self._h, _p(out)), "fri_hip_plan_tiled_rgba_grid", self.ctx)
        return tuple(int(v) for v in out)

    def region(self, x, y, w, h):
        """fri_hip_plan_tiled_rgba_region: (i0, j0, ni, nj), the sub-grid of tiles the region touches. Works on a host-only plan. FriHipError (-1) for an empty
        region or one that leaves the image."""
        out = np.zeros(4, np.uint32)
        _check(load_library().fri_hip_plan_tiled_rgba_region(self._h, x, y, w, h, _p(out)), "fri_hip_plan_tiled_rgba_region", self.ctx)
        return tuple(int(v) for v in out)

    def buffer_tiles(self):
        """fri_hip_plan_tiled_rgba_buffer_tiles: the tiles the plan's (colour, alpha) tile buffers hold room for at the moment."""
        out = np.zeros(2, np.uint64)
        _check(load_library().fri_hip_plan_tiled_rgba_buffer_tiles(self._h, _p(out)), "fri_hip_plan_tiled_rgba_buffer_tiles", self.ctx)
        return int(out[0]), int(out[1])

    # ---- device-pointer entry points (pointers are ints) --------------------------------------------
    def split_tiles_rgba_dev(self, d_rgba, d_colour_tiles, d_alpha_tiles, clean=ALPHA_KEEP, stream=0):
        """fri_hip_split_tiles_rgba_dev (K16): [H][W][4] -> colour_tiles [n][tile_h][tile_w][3] and alpha_tiles [n][tile_h][tile_w] in one pass; ALPHA_CLEAN zeroes
        the colour where A == 0; only enqueues."""
        _check(load_library().fri_hip_split_tiles_rgba_dev(self._h, d_rgba, int(clean), d_colour_tiles, d_alpha_tiles, stream), "fri_hip_split_tiles_rgba_dev", self.ctx)

    def merge_tiles_rgba_dev(self, d_colour_tiles, d_alpha_tiles, d_rgba, stream=0):
        """fri_hip_merge_tiles_rgba_dev (K16): the tile rasters -> [H][W][4], no replicated pixel read; only enqueues."""
        _check(load_library().fri_hip_merge_tiles_rgba_dev(self._h, d_colour_tiles, d_alpha_tiles, d_rgba, stream), "fri_hip_merge_tiles_rgba_dev", self.ctx)

    def merge_tiles_rgba_region_dev(self, d_colour_tiles, d_alpha_tiles, x, y, w, h, d_region, stream=0):
        """fri_hip_merge_tiles_rgba_region_dev (K16): the sub-grid's tile rasters -> the region raster [h][w][4]; only enqueues."""
        _check(load_library().fri_hip_merge_tiles_rgba_region_dev(self._h, d_colour_tiles, d_alpha_tiles, x, y, w, h, d_region, stream), "fri_hip_merge_tiles_rgba_region_dev",
               self.ctx)

    def encode_symbols_tiled_rgba_dev(self, d_rgba, d_params, d_symbols, d_hist, d_oob, d_fit_out_of_range=None, clean=ALPHA_KEEP, qmatrix=None, fit=True, stream=0):
        """fri_hip_encode_symbols_tiled_rgba_dev: the split and the direct stream chain on both inner plans, everything on the device and in plane order: d_params
        float32 [4 n][2][3][6], d_symbols uint16 [n][3][num_some] then [n][num_some], d_hist uint32 [4 n][10][1024], d_oob uint64 [4 n], d_fit_out_of_range uint64
        [4 n] or None. qmatrix is the colour's; alpha always takes ones. Needs set_stream_order()."""
        _check(load_library().fri_hip_encode_symbols_tiled_rgba_dev(self._h, d_rgba, int(clean), _p(_q(qmatrix)), int(bool(fit)), d_params, d_symbols, d_hist, d_oob,
                                                                   d_fit_out_of_range, stream), "fri_hip_encode_symbols_tiled_rgba_dev", self.ctx)

    def decode_region_tiled_rgba_dev(self, d_coefs, x, y, w, h, d_region, qmatrix=None, stream=0):
        """fri_hip_decode_region_tiled_rgba_dev: d_coefs int32, the sub-grid's planes in plane order -> d_region uint8 [h][w][4], device pointers. Refuses a
        capturing stream."""
        _check(load_library().fri_hip_decode_region_tiled_rgba_dev(self._h, d_coefs, _p(_q(qmatrix)), x, y, w, h, d_region, stream), "fri_hip_decode_region_tiled_rgba_dev",
               self.ctx)

    # ---- host-pointer entry points ----------------------------------------------------------------
    def encode_image_tiled_rgba_symbols(self, pixels, qmatrix=None, clean=ALPHA_KEEP):
        """fri_hip_encode_image_tiled_rgba_symbols: (symbols uint16 [4 n][num_some], value_params [4 n][3][6], width_params [4 n][3][6], hist [4 n][10][1024],
        oob [4 n]), all in plane order - what emit.tiled_encode_from_streams_rgba takes; the fit is on. Needs set_stream_order()."""
        px = np.ascontiguousarray(pixels, np.uint8).reshape(-1)
        assert px.size == self.pixel_bytes
        planes = 4 * self.n_tiles
        vp, wp = np.zeros((planes, 3, 6), np.float32), np.zeros((planes, 3, 6), np.float32)
        sym = np.empty((planes, self.num_some), np.uint16)
        hist = np.empty((planes, 10, 1024), np.uint32)
        oob = np.zeros(planes, np.uint64)
        _check(load_library().fri_hip_encode_image_tiled_rgba_symbols(self._h, _p(px), int(clean), _p(_q(qmatrix)), _p(vp), _p(wp), _p(sym), _p(hist), _p(oob)),
               "fri_hip_encode_image_tiled_rgba_symbols", self.ctx)
        return sym, vp, wp, hist, oob

    def decode_image_tiled_rgba(self, coefs, qmatrix=None):
        """fri_hip_decode_image_tiled_rgba: coefs int32 in plane order (what emit.tiled_decode returns for a tiled RGBA file) -> pixels uint8 [H * W * 4]. The
        colour planes go through the inverse kernel with qmatrix and the colour plan's transform and dequantiser, the alpha planes with ones."""
        co = np.ascontiguousarray(coefs, np.int32).reshape(-1)
        assert co.size == self.coef_count
        out = np.empty(self.pixel_bytes, np.uint8)
        _check(load_library().fri_hip_decode_image_tiled_rgba(self._h, _p(co), _p(_q(qmatrix)), _p(out)), "fri_hip_decode_image_tiled_rgba", self.ctx)
        return out

    def decode_region_tiled_rgba(self, coefs, x, y, w, h, qmatrix=None):
        """fri_hip_decode_region_tiled_rgba: coefs int32, the sub-grid's planes in plane order (what emit.tiled_decode_region returns) -> pixels uint8 [h * w * 4]:
        the crop [y : y + h, x : x + w] of what decode_image_tiled_rgba returns for the same file."""
        _, _, ni, nj = self.region(x, y, w, h)
        co = np.ascontiguousarray(coefs, np.int32).reshape(-1)
        assert co.size == ni * nj * self.tile_coef_count
        out = np.empty(w * h * 4, np.uint8)
        _check(load_library().fri_hip_decode_region_tiled_rgba(self._h, _p(co), _p(_q(qmatrix)), x, y, w, h, _p(out)), "fri_hip_decode_region_tiled_rgba", self.ctx)
        return out
