"""ctypes binding of the product's C ABI (include/panoflow.h -> libpanoflow.so).

Used by tests/, bench.py and __graft_entry__.py.  It is plumbing only: every function forwards to the
HIP library and raises if the library or the device is missing -- there is no CPU fallback.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libpanoflow.so")
# the lab build (-DPF_EXPERIMENTS): product sources + the cross-check sweep implementations; loaded by tests and diagnostics only
SO_PATH_EXP = os.path.join(_HERE, "libpanoflow_exp.so")

HINT_UNKNOWN, HINT_RIGHT, HINT_DOWN, HINT_LEFT, HINT_UP = 0, 1, 2, 3, 4


class PanoflowError(RuntimeError):
    pass


class PngCapacityError(PanoflowError):
    """a PNG call's buffer was too small; .needed = the file's size"""

    def __init__(self, msg, needed):
        super().__init__(msg)
        self.needed = needed


def build(force=False):
    """Compile the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", _HERE, "-j8"] + (["-B"] if force else [])
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return SO_PATH


_libs = {}


class Config(C.Structure):
    """pf_config (include/panoflow.h)"""
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("max_cols", C.c_int), ("max_rows", C.c_int), ("stagger_levels", C.c_int),
                ("fuse_small_level_px", C.c_int64), ("fine_gradient_blocks", C.c_int), ("pyramid_chaining", C.c_int), ("sweep_window", C.c_int),
                ("sparse_sweep", C.c_int), ("batch_pairs", C.c_int), ("sweep_wide", C.c_int), ("sweep_wide_threshold", C.c_int), ("sweep_throughput_transposed", C.c_int),
                ("full_width_batch_gradients", C.c_int), ("sweep_impl", C.c_int)]


class SolverParams(C.Structure):
    """pf_solver_params (include/panoflow.h): the constructor arguments of the reference's PixFlow<P> (CPU/PixFlow.hpp:46-68)"""
    _fields_ = [("pyr_scale_factor", C.c_float), ("smoothness_coef", C.c_float), ("vertical_regularization_coef", C.c_float),
                ("horizontal_regularization_coef", C.c_float), ("gradient_step_size", C.c_float), ("downscale_factor", C.c_float),
                ("directional_regularization_coef", C.c_float)]


class JpegParams(C.Structure):
    """pf_jpeg_params (include/panoflow.h)"""
    _fields_ = [("struct_size", C.c_int), ("quality", C.c_int), ("subsampling", C.c_int), ("gpano", C.c_int)]


class ReprojectParams(C.Structure):
    """pf_reproject_params (include/panoflow.h)"""
    _fields_ = [("projection", C.c_int), ("face", C.c_int), ("filter", C.c_int), ("hfov_deg", C.c_double), ("rot", C.c_double * 9)]


class Lens(C.Structure):
    """pf_lens (include/panoflow.h)"""
    _fields_ = [("model", C.c_int), ("filter", C.c_int)] + [(n, C.c_double) for n in ("focal_px", "a", "b", "c", "dd", "shift_x", "shift_y", "min_cos")] + \
               [("crop_cx256", C.c_int), ("crop_cy256", C.c_int), ("crop_r256", C.c_int), ("rot", C.c_double * 9)]


class TiffInfo(C.Structure):
    """pf_tiff_info (include/panoflow.h)"""
    _fields_ = [(n, C.c_int) for n in ("struct_size", "cols", "rows", "samples", "compression", "predictor", "rows_per_strip", "n_strips", "big_endian",
                                        "device_decodable")]


class JpegInfo(C.Structure):
    """pf_jpeg_info (include/panoflow.h)"""
    _fields_ = [(n, C.c_int) for n in ("struct_size", "cols", "rows", "components", "subsampling", "restart_interval", "device_decodable")] + \
               [("reason", C.c_char * 128)]


def lib(exp=False):
    """exp=False: the product library.  exp=True: the lab build with the cross-check sweeps (tests / diagnostics only)."""
    _lib = _libs.get(bool(exp))
    if _lib is None:
        path = SO_PATH_EXP if exp else SO_PATH
        if not os.path.exists(path):
            raise PanoflowError("%s is not built (run __graft_entry__.build()); there is no fallback path" % os.path.basename(path))
        _lib = C.CDLL(path)
        _libs[bool(exp)] = _lib
        _lib.pf_create_cfg.restype = C.c_void_p
        _lib.pf_create_cfg.argtypes = [C.POINTER(Config)]
        _lib.pf_config_init.argtypes = [C.POINTER(Config)]
        _lib.pf_create.restype = C.c_void_p
        _lib.pf_create.argtypes = [C.c_int, C.c_int, C.c_int]
        _lib.pf_destroy.argtypes = [C.c_void_p]
        _lib.pf_last_error.restype = C.c_char_p
        _lib.pf_last_error.argtypes = [C.c_void_p]
        _lib.pf_version.restype = C.c_char_p
        _lib.pf_last_warning.restype = C.c_char_p
        _lib.pf_last_warning.argtypes = [C.c_void_p]
        _lib.pf_warning_count.argtypes = [C.c_void_p]
        _lib.pf_dev_alloc.restype = C.c_void_p
        _lib.pf_dev_alloc.argtypes = [C.c_void_p, C.c_size_t]
        _lib.pf_dev_free.argtypes = [C.c_void_p, C.c_void_p]
        _lib.pf_host_alloc.restype = C.c_void_p
        _lib.pf_host_alloc.argtypes = [C.c_void_p, C.c_size_t]
        _lib.pf_host_free.argtypes = [C.c_void_p, C.c_void_p]
        _lib.pf_algorithmic_bytes.restype = C.c_double
        _lib.pf_level_pixels.restype = C.c_longlong
        _lib.pf_dist_init.restype = C.c_void_p
        _lib.pf_dist_init.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int]
        _lib.pf_dist_destroy.argtypes = [C.c_void_p]
        _lib.pf_dist_last_error.restype = C.c_char_p
        _lib.pf_dist_last_error.argtypes = [C.c_void_p]
        _lib.pf_dist_gather_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        _lib.pf_dist_wait.argtypes = [C.c_void_p]
        _lib.pf_dist_max.argtypes = [C.c_void_p, C.c_void_p]
        _lib.pf_dist_barrier.argtypes = [C.c_void_p]
        _lib.pf_last_swept_steps.restype = C.c_longlong
        _lib.pf_last_swept_steps.argtypes = [C.c_void_p]
        _lib.pf_rig_plan_step.restype = C.c_void_p
        _lib.pf_rig_plan_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        _lib.pf_png_bound.restype = C.c_size_t
        _lib.pf_png_bound.argtypes = [C.c_int, C.c_int]
        _lib.pf_png_segment_bytes.restype = C.c_size_t
        _lib.pf_png_segment_bytes.argtypes = []
        _lib.pf_jpeg_params_init.restype = None
        _lib.pf_jpeg_params_init.argtypes = [C.POINTER(JpegParams)]
        _lib.pf_jpeg_bound.restype = C.c_size_t
        _lib.pf_jpeg_bound.argtypes = [C.c_int, C.c_int, C.POINTER(JpegParams)]
        _lib.pf_jpeg_restart_interval.argtypes = [C.c_int]
        _lib.pf_jpeg_encode_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(JpegParams), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        _lib.pf_jpeg_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(JpegParams), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        _lib.pf_jpeg_encode_batch_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(JpegParams), C.c_void_p, C.c_size_t, C.c_void_p]
        _lib.pf_stitch_result_jpeg.argtypes = [C.c_void_p, C.POINTER(JpegParams), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        _lib.pf_stitch_batch_result_jpeg.argtypes = [C.c_void_p, C.c_int, C.POINTER(JpegParams), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        _lib.pf_tiff_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(TiffInfo)]
        _lib.pf_tiff_set_inflate.argtypes = [C.c_void_p, C.c_int]
        _lib.pf_tiff_device_decodable.argtypes = [C.c_void_p, C.POINTER(TiffInfo)]
        _lib.pf_tiff_decode_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
        _lib.pf_tiff_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
        _lib.pf_tiff_decode_batch_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        _lib.pf_jpeg_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(JpegInfo)]
        _lib.pf_jpeg_decode_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
        _lib.pf_jpeg_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
        _lib.pf_jpeg_decode_batch_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        _lib.pf_stage_jpeg_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        _lib.pf_resize_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]
        _lib.pf_resize.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int]
        _lib.pf_resize_batch_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]
        _lib.pf_stitch_result_resized_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _lib.pf_stitch_batch_result_resized_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _lib.pf_stage_resize_pass.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        rp = C.POINTER(ReprojectParams)
        _lib.pf_reproject_params_init.restype = None
        _lib.pf_reproject_params_init.argtypes = [rp]
        _lib.pf_reproject_rotation.restype = None
        _lib.pf_reproject_rotation.argtypes = [C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double)]
        _lib.pf_reproject_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, rp]
        _lib.pf_reproject.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, rp]
        _lib.pf_reproject_batch_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, rp]
        _lib.pf_reproject_cube_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, rp]
        _lib.pf_stitch_result_reprojected_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, rp, C.c_void_p]
        _lib.pf_stitch_batch_result_reprojected_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, rp, C.c_void_p]
        _lib.pf_stage_reproject_coords.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, rp, C.c_void_p, C.c_void_p]
        ln = C.POINTER(Lens)
        _lib.pf_lens_init.restype = None
        _lib.pf_lens_init.argtypes = [ln, C.c_int]
        _lib.pf_lens_focal.restype = C.c_double
        _lib.pf_lens_focal.argtypes = [C.c_int, C.c_int, C.c_double]
        _lib.pf_lens_rotation.restype = None
        _lib.pf_lens_rotation.argtypes = [C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double)]
        _lib.pf_lens_remap_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, ln]
        _lib.pf_lens_remap.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, ln]
        _lib.pf_lens_remap_batch_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, ln]
        _lib.pf_stage_lens_coords.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, ln, C.c_void_p, C.c_void_p]
    return _lib


EXPORTS = [
    "pf_device_count", "pf_create", "pf_config_init", "pf_create_cfg", "pf_destroy", "pf_last_error", "pf_last_warning", "pf_warning_count", "pf_version", "pf_max_percentage_by_name",
    "pf_solver_params_init", "pf_set_solver_params", "pf_get_solver_params",
    "pf_flow", "pf_flow_bidir", "pf_blend", "pf_novel_view", "pf_stitch_prepare", "pf_stitch_match", "pf_stitch_generate_blend", "pf_stitch_raw_blend", "pf_stitch_gather", "pf_stitch_step", "pf_stitch_prefetch",
    "pf_stitch_step_batch", "pf_stitch_step_batch_dev",
    "pf_stitch_plan_create", "pf_stitch_plan_create_dev", "pf_stitch_plan_destroy", "pf_stitch_plan_info", "pf_stitch_plan_download",
    "pf_stitch_step_planned", "pf_stitch_step_batch_planned", "pf_stitch_step_batch_planned_dev",
    "pf_rig_plan_create", "pf_rig_plan_create_dev", "pf_rig_plan_destroy", "pf_rig_plan_info", "pf_rig_plan_step",
    "pf_rig_stitch_batch", "pf_rig_stitch_batch_dev", "pf_rig_stitch", "pf_rig_stitch_dev", "pf_rig_set_upload_overlap",
    "pf_dev_alloc", "pf_dev_free", "pf_host_alloc", "pf_host_free", "pf_upload", "pf_download", "pf_sync", "pf_checksum_dev", "pf_selftest_packed_chains",
    "pf_flow_bidir_dev", "pf_blend_dev", "pf_novel_view_dev", "pf_novel_view_batch_dev",
    "pf_stage_preprocess", "pf_stage_pyr_down", "pf_stage_gradients", "pf_stage_gauss", "pf_stage_median5", "pf_stage_sweep",
    "pf_stage_diffusion", "pf_stage_upsample_cubic", "pf_stage_final", "pf_stage_adjust_initial_flow", "pf_stage_level",
    "pf_stage_blend_smooth", "pf_stage_tile_blur", "pf_stage_box_blur", "pf_stage_gauss15_form", "pf_stage_level_table",
    "pf_stage_preprocess_batch", "pf_stage_pyramid", "pf_stage_adjust_initial_flow_batch", "pf_stage_intensity_ratio",
    "pf_vis_grey_disparity", "pf_vis_color_wheel", "pf_vis_vector_field", "pf_vis_panel", "pf_vis_panel_dev", "pf_stitch_visualize",
    "pf_png_bound", "pf_png_segment_bytes", "pf_png_encode_dev", "pf_png_encode", "pf_png_encode_batch_dev", "pf_stitch_result_png", "pf_stitch_batch_result_png",
    "pf_jpeg_params_init", "pf_jpeg_bound", "pf_jpeg_restart_interval", "pf_jpeg_encode_dev", "pf_jpeg_encode", "pf_jpeg_encode_batch_dev",
    "pf_stitch_result_jpeg", "pf_stitch_batch_result_jpeg",
    "pf_tiff_probe", "pf_tiff_set_inflate", "pf_tiff_device_decodable", "pf_tiff_decode_dev", "pf_tiff_decode", "pf_tiff_decode_batch_dev",
    "pf_jpeg_probe", "pf_jpeg_decode_dev", "pf_jpeg_decode", "pf_jpeg_decode_batch_dev", "pf_stage_jpeg_decode",
    "pf_resize_dev", "pf_resize", "pf_resize_batch_dev", "pf_stitch_result_resized_dev", "pf_stitch_batch_result_resized_dev", "pf_stage_resize_pass",
    "pf_reproject_params_init", "pf_reproject_rotation", "pf_reproject_dev", "pf_reproject", "pf_reproject_batch_dev", "pf_reproject_cube_dev",
    "pf_stitch_result_reprojected_dev", "pf_stitch_batch_result_reprojected_dev", "pf_stage_reproject_coords",
    "pf_lens_init", "pf_lens_focal", "pf_lens_rotation", "pf_lens_remap_dev", "pf_lens_remap", "pf_lens_remap_batch_dev", "pf_stage_lens_coords",
    "pf_profile_enable", "pf_profile_reset", "pf_profile_count", "pf_profile_get", "pf_algorithmic_bytes", "pf_level_pixels", "pf_last_swept_steps",
    "pf_dist_unique_id", "pf_dist_init", "pf_dist_destroy", "pf_dist_last_error", "pf_dist_gather_async", "pf_dist_wait", "pf_dist_max", "pf_dist_barrier",
]


def _p(a):
    # data_as keeps a reference to the array inside the returned ctypes object, so a converted temporary
    # (_p(_f32(x)) where x needed a copy) stays alive for the duration of the C call
    return a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def _bgra(image):
    """(array, cols, rows, row step): the uint8 BGRA image as it is where its pixels are packed (rows any distance apart), else a contiguous copy"""
    a = np.asarray(image, dtype=np.uint8); rows, cols, _ = a.shape
    if a.strides[2] != 1 or a.strides[1] != 4:
        a = np.ascontiguousarray(a)
    return a, cols, rows, C.c_size_t(a.strides[0])


def _dst(out, cols, rows):
    """(array, row step): the caller's destination array, or a fresh (rows, cols, 4) one"""
    if out is None:
        out = np.empty((max(rows, 0), max(cols, 0), 4), np.uint8)
    return out, C.c_size_t(out.strides[0] if out.ndim == 3 and out.shape[0] > 1 else max(cols, 0) * 4)


def _rows(a, dtype):
    """(array, row step in bytes): the (rows, cols[, channels]) array as it is where the elements of a row are packed (rows any distance
    apart, as in padded[:, :cols]), else a contiguous copy -- _bgra() for planes of any type"""
    a = np.asarray(a, dtype=dtype)
    inner = a.itemsize
    for ax in range(a.ndim - 1, 0, -1):
        if a.strides[ax] != inner:
            a = np.ascontiguousarray(a)
            break
        inner *= a.shape[ax]
    if a.shape[0] > 1 and a.strides[0] < inner:
        a = np.ascontiguousarray(a)
    return a, (a.strides[0] if a.shape[0] > 1 else inner)


def _shared(planes, dtype):
    """(arrays, c_size_t step) of planes that go behind ONE step argument (L and R, the two flows, a rig's images): as they are where
    their rows are the same distance apart, else contiguous copies"""
    rs = [_rows(a, dtype) for a in planes]
    if len(set(st for _, st in rs)) > 1:
        rs = [_rows(np.ascontiguousarray(a), dtype) for a, _ in rs]
    return [a for a, _ in rs], C.c_size_t(rs[0][1] if rs else 0)


def _like(shape, dtype, step):
    """a fresh plane of `shape` whose rows are `step` bytes apart (what an output that shares an input's step argument needs)"""
    row = int(np.prod(shape[1:])) * np.dtype(dtype).itemsize
    buf = np.empty((shape[0], max(int(step), row)), np.uint8)
    strides, inner = [buf.strides[0]], row
    for n in shape[1:]:
        inner //= n
        strides.append(inner)
    return np.ndarray(tuple(shape), dtype, buffer=buf, strides=tuple(strides))


def _outs(outs, shape, dtype):
    """(arrays, c_size_t step): the caller's destination arrays (None: fresh ones) of one shape behind one step argument; a given array
    keeps its row stride, its rows' elements must be packed and all given arrays must share the stride"""
    outs = [np.empty(shape, dtype) if o is None else o for o in outs]
    steps = set()
    for o in outs:
        assert o.dtype == np.dtype(dtype) and o.shape == tuple(shape), "destination of shape %r / %s expected" % (tuple(shape), np.dtype(dtype))
        a, st = _rows(o, dtype)
        assert a is o or np.shares_memory(a, o), "the elements of a destination's rows must be packed"
        steps.add(st)
    assert len(steps) <= 1, "destinations behind one step argument must share their row stride"
    return outs, C.c_size_t(steps.pop() if steps else 0)


def _dptrs(v, n=None):
    """sequence of device pointers (ints; 0 or None: NULL) -> c_void_p array of n entries (default len(v)); a shorter v leaves NULLs"""
    return (C.c_void_p * max(len(v) if n is None else n, 1))(*[C.c_void_p(int(x)) if x else None for x in v])


def _ref(params):
    return C.byref(params) if params is not None else None


def max_percentage_by_name(name):
    """makeOpticalFlowByName (CPU/PixFlow.hpp:459-500): raises on an unknown algorithm name."""
    v = lib().pf_max_percentage_by_name(name.encode())
    if v < 0:
        raise PanoflowError(lib().pf_last_error(None).decode())
    return v


def png_bound(cols, rows):
    """capacity that holds the PNG of any cols x rows image (pf_png_bound)"""
    return int(lib().pf_png_bound(cols, rows))


def jpeg_params(quality=None, subsampling=None, gpano=None):
    """a JpegParams with the library's defaults (pf_jpeg_params_init) and the given fields over them"""
    p = JpegParams()
    lib().pf_jpeg_params_init(C.byref(p))
    for name, v in (("quality", quality), ("subsampling", subsampling), ("gpano", gpano)):
        if v is not None:
            setattr(p, name, int(v))
    return p


def jpeg_bound(cols, rows, params=None):
    """capacity that holds the JPEG of any cols x rows image (pf_jpeg_bound); 0 for a shape the encoder refuses"""
    return int(lib().pf_jpeg_bound(cols, rows, C.byref(params) if params is not None else None))


def jpeg_restart_interval(subsampling):
    """MCUs per restart interval of the device JPEG encoder (pf_jpeg_restart_interval)"""
    return int(lib().pf_jpeg_restart_interval(subsampling))


# PF_RESIZE_* (Pillow's numbering of its resampling filters)
RESIZE_LANCZOS, RESIZE_BILINEAR, RESIZE_BICUBIC, RESIZE_BOX, RESIZE_HAMMING = 1, 2, 3, 4, 5


# PF_PROJ_*, PF_FACE_*, PF_REPROJECT_*
PROJ_CUBE, PROJ_RECTILINEAR, PROJ_EQUIRECT = 0, 1, 2
FACE_FRONT, FACE_RIGHT, FACE_BACK, FACE_LEFT, FACE_UP, FACE_DOWN = range(6)
FACE_NAMES = ("front", "right", "back", "left", "up", "down")
REPROJECT_BILINEAR, REPROJECT_BICUBIC = 2, 3


def reproject_rotation(yaw_deg=0.0, pitch_deg=0.0, roll_deg=0.0):
    """the nine doubles of Rz(yaw) Ry(-pitch) Rx(roll), row-major (pf_reproject_rotation: host only)"""
    r = (C.c_double * 9)()
    lib().pf_reproject_rotation(float(yaw_deg), float(pitch_deg), float(roll_deg), r)
    return list(r)


def reproject_params(projection=None, face=None, filter=None, hfov_deg=None, rot=None):
    """a ReprojectParams with the library's defaults (pf_reproject_params_init) and the given fields over them"""
    p = ReprojectParams()
    lib().pf_reproject_params_init(C.byref(p))
    for name, v in (("projection", projection), ("face", face), ("filter", filter)):
        if v is not None:
            setattr(p, name, int(v))
    if hfov_deg is not None:
        p.hfov_deg = float(hfov_deg)
    if rot is not None:
        for k, v in enumerate(rot):
            p.rot[k] = float(v)
    return p


# PF_LENS_*
LENS_RECTILINEAR, LENS_FISHEYE_EQUIDISTANT, LENS_FISHEYE_STEREOGRAPHIC, LENS_FISHEYE_EQUISOLID = range(4)


def lens_focal(model, photo_cols, hfov_deg):
    """focal_px of a photo photo_cols wide spanning hfov_deg degrees across (pf_lens_focal: host only)"""
    return lib().pf_lens_focal(int(model), int(photo_cols), float(hfov_deg))


def lens_rotation(yaw_deg=0.0, pitch_deg=0.0, roll_deg=0.0):
    """the rot of a camera posed by reproject_rotation(yaw, pitch, roll): its transpose (pf_lens_rotation: host only)"""
    r = (C.c_double * 9)()
    lib().pf_lens_rotation(float(yaw_deg), float(pitch_deg), float(roll_deg), r)
    return list(r)


def lens(model, filter=None, rot=None, **fields):
    """a Lens with the library's defaults for the model (pf_lens_init) and the given fields over them"""
    p = Lens()
    lib().pf_lens_init(C.byref(p), int(model))
    if filter is not None:
        p.filter = int(filter)
    for name, v in fields.items():
        setattr(p, name, int(v) if name.startswith("crop_") else float(v))
    if rot is not None:
        for k, v in enumerate(rot):
            p.rot[k] = float(v)
    return p


def tiff_probe(data):
    """TiffInfo of the first IFD of a TIFF file's bytes (pf_tiff_probe: host only, no device needed); raises on a refusal"""
    buf = np.frombuffer(bytes(data) or b"\0", np.uint8)   # (an empty file is still a pointer and a length of 0)
    info = TiffInfo(); info.struct_size = C.sizeof(TiffInfo)
    if lib().pf_tiff_probe(None, _p(buf), C.c_size_t(len(data)), C.byref(info)) != 0:
        raise PanoflowError(lib().pf_last_error(None).decode())
    return info


def tiff_device_decodable(info, ctx=None):
    """would the decode calls of `ctx` (a Context; None: default settings) take the probed file?  (pf_tiff_device_decodable)"""
    return bool(lib().pf_tiff_device_decodable(ctx.h if ctx is not None else None, C.byref(info)))


def jpeg_probe(data):
    """JpegInfo of a JPEG file's bytes (pf_jpeg_probe: host only, no device needed).  device_decodable says whether the decode calls
    take the file and `reason` why not; raises only for bytes that do not begin as a JPEG"""
    buf = np.frombuffer(bytes(data) or b"\0", np.uint8)
    info = JpegInfo(); info.struct_size = C.sizeof(JpegInfo)
    if lib().pf_jpeg_probe(None, _p(buf), C.c_size_t(len(data)), C.byref(info)) != 0:
        raise PanoflowError(lib().pf_last_error(None).decode())
    return info


def png_segment_bytes():
    """bytes of filtered scanlines one deflate segment covers (pf_png_segment_bytes)"""
    return int(lib().pf_png_segment_bytes())


def algorithmic_bytes(cols, rows):
    return float(lib().pf_algorithmic_bytes(cols, rows))


def level_pixels(cols, rows):
    n = C.c_int(0); s = C.c_longlong(0)
    p = lib().pf_level_pixels(cols, rows, C.byref(n), C.byref(s))
    return int(p), n.value, int(s.value)


def dist_unique_id():
    """rank 0: the 128-byte ncclUniqueId every rank passes to Dist()"""
    buf = C.create_string_buffer(128)
    if lib().pf_dist_unique_id(buf) != 0:
        raise PanoflowError("pf_dist_unique_id: " + lib().pf_dist_last_error(None).decode())
    return buf.raw


class Dist:
    """The path's only exchange: gather of per-pair results into rank 0's HBM over RCCL (pf_dist_*), asynchronous."""

    def __init__(self, device, unique_id, rank, world):
        self.l = lib()
        h = self.l.pf_dist_init(device, C.c_char_p(unique_id), rank, world)
        if not h:
            raise PanoflowError("pf_dist_init failed: " + self.l.pf_dist_last_error(None).decode())
        self.h = C.c_void_p(h); self.rank = rank; self.world = world

    def _chk(self, rc):
        if rc != 0:
            raise PanoflowError("pf_dist error %d: %s" % (rc, self.l.pf_dist_last_error(self.h).decode()))

    def gather_async(self, d_send, d_recv_all, nbytes):
        self._chk(self.l.pf_dist_gather_async(self.h, C.c_void_p(d_send), C.c_void_p(d_recv_all) if d_recv_all else None, C.c_size_t(nbytes)))

    def wait(self):
        self._chk(self.l.pf_dist_wait(self.h))

    def max(self, value):
        v = C.c_double(value)
        self._chk(self.l.pf_dist_max(self.h, C.byref(v)))
        return v.value

    def barrier(self):
        self._chk(self.l.pf_dist_barrier(self.h))

    def close(self):
        if self.h:
            self.l.pf_dist_destroy(self.h)
            self.h = None


class StitchPlan:
    """pf_stitch_plan: one rig's overlap map and blend ramp in HBM (Context.stitch_plan).  Owned by its context; close() frees it early."""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, C.c_void_p(handle)
        cols, rows, ov = C.c_int(0), C.c_int(0), C.c_longlong(0)
        ctx._chk(ctx.l.pf_stitch_plan_info(self.h, C.byref(cols), C.byref(rows), C.byref(ov)))
        self.cols, self.rows, self.overlap_px = cols.value, rows.value, ov.value

    def download(self):
        """(Map (rows, cols) uint8, finished ramp (rows, cols) float32)"""
        mp = np.empty((self.rows, self.cols), np.uint8); bl = np.empty((self.rows, self.cols), np.float32)
        self.ctx._chk(self.ctx.l.pf_stitch_plan_download(self.ctx.h, self.h, _p(mp), C.c_size_t(self.cols), _p(bl), C.c_size_t(self.cols * 4)))
        return mp, bl

    def close(self):
        if self.h and self.ctx.h:
            self.ctx._chk(self.ctx.l.pf_stitch_plan_destroy(self.ctx.h, self.h))
        self.h = None


class RigPlan:
    """pf_rig_plan: the stitch plans of every step of one rig's chain (Context.rig_plan).  .steps are StitchPlan objects the rig owns
    (usable wherever a plan is; closing one raises); close() frees the rig and its steps early."""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, C.c_void_p(handle)
        n, cols, rows = C.c_int(0), C.c_int(0), C.c_int(0)
        ctx._chk(ctx.l.pf_rig_plan_info(self.h, C.byref(n), C.byref(cols), C.byref(rows)))
        self.n_steps, self.cols, self.rows = n.value, cols.value, rows.value
        self.steps = []
        for i in range(self.n_steps):
            h = ctx.l.pf_rig_plan_step(ctx.h, self.h, i)
            if not h:
                ctx._chk(-1)
            self.steps.append(StitchPlan(ctx, h))

    def close(self):
        if self.h and self.ctx.h:
            self.ctx._chk(self.ctx.l.pf_rig_plan_destroy(self.ctx.h, self.h))
            for p in self.steps:
                p.h = None
        self.h = None


class Context:
    def __init__(self, device=0, max_cols=0, max_rows=0, exp=False, **knobs):
        """knobs: fields of pf_config (stagger_levels, fuse_small_level_px, sweep_window, sparse_sweep, sweep_impl, ...);
        exp=True loads the lab build, the only one that accepts sweep_impl 1 (the v1 cross-check kernel) and sweep_wide 1."""
        self.l = lib(exp)
        if knobs:
            cfg = Config()
            self.l.pf_config_init(C.byref(cfg))
            cfg.device, cfg.max_cols, cfg.max_rows = device, max_cols, max_rows
            for k, v in knobs.items():
                if not hasattr(cfg, k):
                    raise TypeError("unknown pf_config field %r" % k)
                setattr(cfg, k, v)
            h = self.l.pf_create_cfg(C.byref(cfg))
        else:
            h = self.l.pf_create(device, max_cols, max_rows)
        if not h:
            raise PanoflowError("pf_create failed: " + self.l.pf_last_error(None).decode())
        self.h = C.c_void_p(h)  # keep it a c_void_p: a bare int would be passed as a 32-bit C int

    def close(self):
        if self.h:
            for p in getattr(self, "_pinned", []):
                self.l.pf_host_free(self.h, C.c_void_p(p))
            self._pinned = []
            self.l.pf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise PanoflowError("panoflow error %d: %s" % (rc, self.l.pf_last_error(self.h).decode()))

    # ---- host-buffer entry points ----
    # Images, flows, blend planes and maps may be views whose rows are any distance apart (padded[:, :cols]): they are passed in place with
    # their row step.  Planes that share one step argument of the C call are passed in place where their strides agree, else as copies.
    # out= (where a method has it) takes destination arrays, whose row stride is kept; the default is a fresh packed array, as before.
    def flow(self, i0, i1, max_pct, hint, out=None):
        (a, b), step = _shared([i0, i1], np.uint8); rows, cols, _ = a.shape
        (out,), fstep = _outs([out], (rows, cols, 2), np.float32)
        self._chk(self.l.pf_flow(self.h, _p(a), _p(b), cols, rows, step, max_pct, hint, _p(out), fstep))
        return out

    def flow_bidir(self, L, R, max_pct, out=None):
        """out: (flow_l2r, flow_r2l) destination arrays of one row stride"""
        (a, b), step = _shared([L, R], np.uint8); rows, cols, _ = a.shape
        (f0, f1), fstep = _outs(out if out is not None else [None, None], (rows, cols, 2), np.float32)
        self._chk(self.l.pf_flow_bidir(self.h, _p(a), _p(b), cols, rows, step, max_pct, _p(f0), _p(f1), fstep))
        return f0, f1

    def blend(self, L, R, f_l2r, f_r2l, blend, out=None):
        (a, b), step = _shared([L, R], np.uint8); rows, cols, _ = a.shape
        (f0, f1), fstep = _shared([f_l2r, f_r2l], np.float32)
        bl, bstep = _rows(blend, np.float32)
        (out,), ostep = _outs([out], (rows, cols, 4), np.uint8)
        self._chk(self.l.pf_blend(self.h, _p(a), _p(b), step, _p(f0), _p(f1), fstep, _p(bl), C.c_size_t(bstep), cols, rows, _p(out), ostep))
        return out

    def novel_view(self, L, R, max_pct, blend, want_flows=True, out=None, flows_out=None):
        """flows_out: (flow_l2r, flow_r2l) destination arrays of one row stride (implies want_flows)"""
        (a, b), step = _shared([L, R], np.uint8); rows, cols, _ = a.shape
        bl, bstep = _rows(blend, np.float32)
        (out,), ostep = _outs([out], (rows, cols, 4), np.uint8)
        f0 = f1 = None; fstep = C.c_size_t(cols * 8)
        if want_flows or flows_out is not None:
            (f0, f1), fstep = _outs(flows_out if flows_out is not None else [None, None], (rows, cols, 2), np.float32)
        self._chk(self.l.pf_novel_view(self.h, _p(a), _p(b), cols, rows, step, max_pct, _p(bl), C.c_size_t(bstep), _p(out), ostep,
                                       _p(f0) if f0 is not None else None, _p(f1) if f1 is not None else None, fstep))
        return out, f0, f1

    def stitch_prepare(self, L, R):
        """(map, overlapped L, overlapped R, blend ramp, MergedDis); the overlapped images come at the inputs' row stride (the C call's rule)"""
        (a, b), step = _shared([L, R], np.uint8); rows, cols, _ = a.shape
        mp = np.empty((rows, cols), np.uint8); ovl = _like(a.shape, np.uint8, step.value); ovr = _like(a.shape, np.uint8, step.value)
        bl = np.empty((rows, cols), np.float32); md = np.empty((rows, cols), np.float32)
        self._chk(self.l.pf_stitch_prepare(self.h, _p(a), _p(b), cols, rows, step, _p(mp), C.c_size_t(cols), _p(ovl), _p(ovr), _p(bl),
                                           C.c_size_t(cols * 4), _p(md)))
        return mp, ovl, ovr, bl, md

    def stitch_match(self, L, R):
        """MatchImages + overlap masking only"""
        (a, b), step = _shared([L, R], np.uint8); rows, cols, _ = a.shape
        mp = np.empty((rows, cols), np.uint8); ovl = _like(a.shape, np.uint8, step.value); ovr = _like(a.shape, np.uint8, step.value)
        self._chk(self.l.pf_stitch_match(self.h, _p(a), _p(b), cols, rows, step, _p(mp), C.c_size_t(cols), _p(ovl), _p(ovr)))
        return mp, ovl, ovr

    def stitch_generate_blend(self, mp):
        """GenerateBlend from a given map (the reference reads its public Map member)"""
        m, mstep = _rows(mp, np.uint8); rows, cols = m.shape
        bl = np.empty((rows, cols), np.float32); md = np.empty((rows, cols), np.float32)
        self._chk(self.l.pf_stitch_generate_blend(self.h, _p(m), C.c_size_t(mstep), cols, rows, _p(bl), C.c_size_t(cols * 4), _p(md)))
        return bl, md

    def stitch_raw_blend(self, L, R):
        """GenerateBlend before its smoothing (what countblend returns in the overlap) + MergedDis."""
        (a, b), step = _shared([L, R], np.uint8); rows, cols, _ = a.shape
        bl = np.empty((rows, cols), np.float32); md = np.empty((rows, cols), np.float32)
        self._chk(self.l.pf_stitch_raw_blend(self.h, _p(a), _p(b), cols, rows, step, _p(bl), C.c_size_t(cols * 4), _p(md)))
        return bl, md

    def stitch_gather(self, L, R, merged, mp, out=None):
        (a, b, g), step = _shared([L, R, merged], np.uint8); rows, cols, _ = a.shape
        m, mstep = _rows(mp, np.uint8)
        (out,), ostep = _outs([out], (rows, cols, 4), np.uint8)
        self._chk(self.l.pf_stitch_gather(self.h, _p(a), _p(b), _p(g), step, _p(m), C.c_size_t(mstep), cols, rows, _p(out), ostep))
        return out

    def stitch_prefetch(self, next_L):
        """announce the NEXT stitch_step's left image (a uint8 array with packed pixels, rows any distance apart, kept alive and unchanged
        until then)"""
        if next_L is None:
            self._chk(self.l.pf_stitch_prefetch(self.h, None, 0, 0, C.c_size_t(0)))
            return
        a, step = _rows(next_L, np.uint8)
        assert a is next_L, "the announced image is read in place: a uint8 array whose pixels are packed"
        rows, cols, _ = next_L.shape
        self._chk(self.l.pf_stitch_prefetch(self.h, _p(next_L), cols, rows, C.c_size_t(step)))

    def stitch_plan(self, L, R):
        """The plan of a step whose alpha masks are L's and R's (only alpha matters); R=None takes the R mask from the composite the
        last stitch_step left in HBM."""
        ims, step = _shared([L] if R is None else [L, R], np.uint8); rows, cols, _ = ims[0].shape
        h = C.c_void_p(None)
        self._chk(self.l.pf_stitch_plan_create(self.h, _p(ims[0]), None if R is None else _p(ims[1]), cols, rows, step, C.byref(h)))
        return StitchPlan(self, h.value)

    def stitch_plan_dev(self, d_l, d_r, cols, rows):
        h = C.c_void_p(None)
        self._chk(self.l.pf_stitch_plan_create_dev(self.h, C.c_void_p(d_l), C.c_void_p(d_r), cols, rows, C.byref(h)))
        return StitchPlan(self, h.value)

    def rig_plan(self, top, Ls):
        """The plans of the whole chain top, Ls[0], Ls[1], ... (only alphas matter): RigPlan"""
        ims, step = _shared([top] + list(Ls), np.uint8); rows, cols, _ = ims[0].shape
        assert all(a.shape == (rows, cols, 4) for a in ims)
        arr = (C.c_void_p * max(len(ims) - 1, 1))(*[a.ctypes.data for a in ims[1:]])
        h = C.c_void_p(None)
        self._chk(self.l.pf_rig_plan_create(self.h, len(ims) - 1, _p(ims[0]), arr, cols, rows, step, C.byref(h)))
        return RigPlan(self, h.value)

    def rig_plan_dev(self, d_top, d_ls, cols, rows):
        h = C.c_void_p(None)
        self._chk(self.l.pf_rig_plan_create_dev(self.h, len(d_ls), C.c_void_p(d_top), _dptrs(d_ls), cols, rows, C.byref(h)))
        return RigPlan(self, h.value)

    def rig_stitch_batch(self, rig, tops, Ls, max_pct, in_flight=8, want=None, out=None):
        """The whole chain of len(tops) frames of the rig: Ls[k] = frame k's left images in chain order.  Returns outs[k][i], the
        composite after step i + 1 of frame k; want(k, i) -> bool selects what is downloaded (default all; None where not), out[k][i]
        are optional preallocated (rows, cols, 4) uint8 arrays of one row stride (None entries skip).  Raises as a whole if any frame is off the rig."""
        n, ns = len(tops), rig.n_steps
        rows, cols = rig.rows, rig.cols
        assert len(Ls) == n and all(len(r) == ns for r in Ls)
        ims, step = _shared(list(tops) + [a for row in Ls for a in row], np.uint8)
        assert all(a.shape == (rows, cols, 4) for a in ims)
        ts, ls = ims[:n], ims[n:]
        if out is not None:
            outs = [list(r) for r in out]
            given, ostep = _outs([o for r in outs for o in r if o is not None], (rows, cols, 4), np.uint8)
            if not given:
                ostep = C.c_size_t(cols * 4)
        else:
            outs = [[np.empty((rows, cols, 4), np.uint8) if want is None or want(k, i) else None for i in range(ns)] for k in range(n)]
            ostep = C.c_size_t(cols * 4)
        ptrs = lambda v: (C.c_void_p * max(len(v), 1))(*[a.ctypes.data if a is not None else None for a in v])
        self._chk(self.l.pf_rig_stitch_batch(self.h, rig.h, n, ptrs(ts), ptrs(ls), cols, rows, step, max_pct, ptrs([o for r in outs for o in r]), ostep, in_flight))
        return outs

    def rig_set_upload_overlap(self, on):
        """rig_stitch_batch, calls of more than two waves: the later waves' second upload beside the compute (default) or between the waves"""
        self._chk(self.l.pf_rig_set_upload_overlap(self.h, int(bool(on))))

    def rig_stitch_batch_dev(self, rig, d_tops, d_ls, max_pct, d_outs, in_flight=8):
        """the device form: d_tops[k], d_ls[k][i], d_outs[k][i] device pointers (packed BGRA); only d_outs[k][-1] must be given"""
        self._chk(self.l.pf_rig_stitch_batch_dev(self.h, rig.h, len(d_tops), _dptrs(d_tops), _dptrs([x for r in d_ls for x in r]), rig.cols, rig.rows, max_pct,
                                                 _dptrs([x for r in d_outs for x in r]), in_flight))

    def stitch_step(self, L, R, max_pct, want_out=True, out=None, plan=None):
        """One iteration of main.cpp's loop on the device; R=None chains on the previous result kept in HBM.
        out: optional preallocated (rows, cols, 4) uint8 array for the composite, rows any distance apart (a caller that reuses its buffer,
        like the reference's Mat, does not pay a fresh 144 MB allocation + first-touch page faults per call).
        plan: a StitchPlan of these masks -- the same bytes without recomputing the map and the ramp; raises if the masks differ."""
        ims, step = _shared([L] if R is None else [L, R], np.uint8); rows, cols, _ = ims[0].shape   # named, so that a converted copy outlives the call
        ostep = C.c_size_t(cols * 4)
        if out is not None or want_out:
            (out,), ostep = _outs([out], (rows, cols, 4), np.uint8)
        fn = self.l.pf_stitch_step if plan is None else self.l.pf_stitch_step_planned
        self._chk(fn(*([self.h] + ([] if plan is None else [plan.h]) + [_p(ims[0]), None if R is None else _p(ims[1]), cols, rows, step, max_pct,
                                                                       None if out is None else _p(out), ostep])))
        self._step_shape = (rows, cols)
        return out

    def stitch_step_batch(self, Ls, Rs, max_pct, in_flight=8, want_out=True, out=None, plan=None):
        """n independent stitch steps of one size (frame k = one stitch_step of its own chain).  Rs=None, or a None entry, chains
        frame k on its composite from the previous stitch_step_batch call.  Returns a list of (rows, cols, 4) arrays, or of None.
        out: optional list of preallocated (rows, cols, 4) uint8 arrays of one row stride for the composites (as stitch_step's `out`)."""
        n = len(Ls)
        given = [] if Rs is None else [r for r in Rs if r is not None]
        assert Rs is None or len(Rs) == n
        ims, step = _shared(list(Ls) + given, np.uint8)
        ls = ims[:n]
        rows, cols = ls[0].shape[:2] if n else (0, 0)
        assert all(a.shape == (rows, cols, 4) for a in ims)
        it = iter(ims[n:])
        rs = None if Rs is None else [None if r is None else next(it) for r in Rs]
        ostep = C.c_size_t(cols * 4)
        if out is not None:
            assert len(out) == n
            outs, ostep = _outs(list(out), (rows, cols, 4), np.uint8)
            want_out = True
        else:
            outs = [np.empty((rows, cols, 4), np.uint8) for _ in range(n)] if want_out else [None] * n
        arr = lambda v: (C.c_void_p * max(n, 1))(*[a.ctypes.data if a is not None else None for a in v])
        if plan is not None:   # one plan for all frames; the call raises as a whole if any frame's masks differ from it
            self._chk(self.l.pf_stitch_step_batch_planned(self.h, plan.h, n, arr(ls), None if rs is None else arr(rs), cols, rows, step,
                                                          max_pct, arr(outs) if want_out else None, ostep, in_flight))
        else:
            self._chk(self.l.pf_stitch_step_batch(self.h, n, arr(ls), None if rs is None else arr(rs), cols, rows, step, max_pct,
                                                  arr(outs) if want_out else None, ostep, in_flight))
        return outs

    def stitch_step_batch_dev(self, d_l, d_r, cols, rows, max_pct, d_out, in_flight=8, plan=None):
        """the device form: lists of device pointers (packed BGRA), every d_r entry non-NULL"""
        n = len(d_l)
        if plan is not None:
            self._chk(self.l.pf_stitch_step_batch_planned_dev(self.h, plan.h, n, _dptrs(d_l), _dptrs(d_r, n), cols, rows, max_pct, _dptrs(d_out, n), in_flight))
        else:
            self._chk(self.l.pf_stitch_step_batch_dev(self.h, n, _dptrs(d_l), _dptrs(d_r, n), cols, rows, max_pct, _dptrs(d_out, n), in_flight))

    # ---- flow visualisation (CPU/OpticalFlow.cpp:147-204, the panel of CPU/main.cpp:20-45) ----
    def vis_grey_disparity(self, flow, out=None):
        """visualizeFlowAsGreyDisparity: (rows, cols) uint8"""
        f, fstep = _rows(flow, np.float32); rows, cols, _ = f.shape
        (out,), ostep = _outs([out], (rows, cols), np.uint8)
        self._chk(self.l.pf_vis_grey_disparity(self.h, _p(f), C.c_size_t(fstep), cols, rows, _p(out), ostep))
        return out

    def vis_color_wheel(self, flow, out=None):
        """visualizeFlowColorWheel: (rows, cols, 3) uint8 BGR"""
        f, fstep = _rows(flow, np.float32); rows, cols, _ = f.shape
        (out,), ostep = _outs([out], (rows, cols, 3), np.uint8)
        self._chk(self.l.pf_vis_color_wheel(self.h, _p(f), C.c_size_t(fstep), cols, rows, _p(out), ostep))
        return out

    def vis_vector_field(self, flow, image, out=None):
        """visualizeFlowAsVectorField: (rows, cols, 4) uint8 BGRA, the image with the flow's arrows"""
        f, fstep = _rows(flow, np.float32); im, istep = _rows(image, np.uint8); rows, cols, _ = f.shape
        (out,), ostep = _outs([out], (rows, cols, 4), np.uint8)
        self._chk(self.l.pf_vis_vector_field(self.h, _p(f), C.c_size_t(fstep), _p(im), C.c_size_t(istep), cols, rows, _p(out), ostep))
        return out

    def vis_panel(self, flow, image, out=None):
        """buildvisualizations' strip of one direction: (rows, 3 * cols, 4) uint8 BGRA"""
        f, fstep = _rows(flow, np.float32); im, istep = _rows(image, np.uint8); rows, cols, _ = f.shape
        (out,), ostep = _outs([out], (rows, 3 * cols, 4), np.uint8)
        self._chk(self.l.pf_vis_panel(self.h, _p(f), C.c_size_t(fstep), _p(im), C.c_size_t(istep), cols, rows, _p(out), ostep))
        return out

    def vis_panel_dev(self, d_flow, d_image, cols, rows, d_out):
        self._chk(self.l.pf_vis_panel_dev(self.h, C.c_void_p(d_flow), C.c_void_p(d_image), cols, rows, C.c_void_p(d_out)))

    def stitch_visualize(self, shape=None, out=None):
        """the (L->R, R->L) panels of the last stitch_step from what it left in HBM; shape = (rows, cols) of that step (default: the last
        stitch_step made through this object); out: the two destination arrays, of one row stride"""
        rows, cols = shape if shape is not None else self._step_shape
        (a, b), step = _outs(out if out is not None else [None, None], (rows, 3 * cols, 4), np.uint8)
        self._chk(self.l.pf_stitch_visualize(self.h, _p(a), _p(b), step))
        return a, b

    # ---- PNG files made on the device (pf_png_*): every method returns the file as bytes ----
    def _file_call(self, bound, cols, rows, call, cap, *pr):
        """call(*pr, buffer, cap, size_ref) -> rc, where pr is the params reference of a format that takes one.  cap=None: bound(cols, rows, *pr).
        A short buffer raises PngCapacityError carrying the needed size."""
        cap = int(bound(cols, rows, *pr)) if cap is None else int(cap)
        buf = np.empty(max(cap, 1), np.uint8); size = C.c_size_t(0)
        rc = call(*pr, _p(buf), C.c_size_t(cap), C.byref(size))
        if rc != 0 and 0 < cap < size.value:
            raise PngCapacityError("panoflow error %d: %s" % (rc, self.l.pf_last_error(self.h).decode()), size.value)
        self._chk(rc)
        return buf[:size.value].tobytes()

    def _file_batch_call(self, bound, encode, d_bgra, cols, rows, *pr):
        """encode(handle, n, sources, cols, rows, *pr, buffers, cap_each, sizes) -> rc: n files into buffers of bound(cols, rows, *pr) bytes"""
        n = len(d_bgra)
        cap = int(bound(cols, rows, *pr))
        bufs = [np.empty(max(cap, 1), np.uint8) for _ in range(n)]
        outs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs]); sizes = (C.c_size_t * n)()
        self._chk(encode(self.h, n, _dptrs(d_bgra), cols, rows, *pr, outs, C.c_size_t(cap), sizes))
        return [bufs[k][:sizes[k]].tobytes() for k in range(n)]

    def png_encode(self, image, cap=None):
        """host BGRA (rows, cols, 4) array, any row stride -> PNG file bytes"""
        a, cols, rows, step = _bgra(image)
        return self._file_call(self.l.pf_png_bound, cols, rows, lambda b, c, s: self.l.pf_png_encode(self.h, _p(a), step, cols, rows, b, c, s), cap)

    def png_encode_dev(self, d_bgra, cols, rows, cap=None):
        return self._file_call(self.l.pf_png_bound, cols, rows, lambda b, c, s: self.l.pf_png_encode_dev(self.h, C.c_void_p(d_bgra), cols, rows, b, c, s), cap)

    def png_encode_batch_dev(self, d_bgra, cols, rows):
        """n same-size device images -> list of n files"""
        return self._file_batch_call(self.l.pf_png_bound, self.l.pf_png_encode_batch_dev, d_bgra, cols, rows)

    def stitch_result_png(self, shape=None, cap=None):
        """the PNG of the composite the last stitch_step left in HBM; shape = (rows, cols) of that step (default: the last stitch_step made
        through this object), used only to size the buffer"""
        rows, cols = shape if shape is not None else getattr(self, "_step_shape", (1, 1))
        return self._file_call(self.l.pf_png_bound, cols, rows, lambda b, c, s: self.l.pf_stitch_result_png(self.h, b, c, s), cap)

    def stitch_batch_result_png(self, frame, shape, cap=None):
        """the PNG of frame slot `frame` of the last stitch_step_batch; shape = (rows, cols) of that call"""
        rows, cols = shape
        return self._file_call(self.l.pf_png_bound, cols, rows, lambda b, c, s: self.l.pf_stitch_batch_result_png(self.h, frame, b, c, s), cap)

    # ---- JPEG files made on the device (pf_jpeg_*): every method returns the file as bytes; params = a JpegParams or None (defaults) ----
    def jpeg_encode(self, image, params=None, cap=None):
        """host BGRA (rows, cols, 4) array, any row stride -> JPEG file bytes"""
        a, cols, rows, step = _bgra(image)
        return self._file_call(self.l.pf_jpeg_bound, cols, rows, lambda pr, b, c, s: self.l.pf_jpeg_encode(self.h, _p(a), step, cols, rows, pr, b, c, s), cap, _ref(params))

    def jpeg_encode_dev(self, d_bgra, cols, rows, params=None, cap=None):
        return self._file_call(self.l.pf_jpeg_bound, cols, rows, lambda pr, b, c, s: self.l.pf_jpeg_encode_dev(self.h, C.c_void_p(d_bgra), cols, rows, pr, b, c, s), cap, _ref(params))

    def jpeg_encode_batch_dev(self, d_bgra, cols, rows, params=None):
        """n same-size device images -> list of n files"""
        return self._file_batch_call(self.l.pf_jpeg_bound, self.l.pf_jpeg_encode_batch_dev, d_bgra, cols, rows, _ref(params))

    def stitch_result_jpeg(self, params=None, shape=None, cap=None):
        """the JPEG of the composite the last stitch_step left in HBM; shape = (rows, cols) of that step (default: the last stitch_step made
        through this object), used only to size the buffer"""
        rows, cols = shape if shape is not None else getattr(self, "_step_shape", (1, 1))
        return self._file_call(self.l.pf_jpeg_bound, cols, rows, lambda pr, b, c, s: self.l.pf_stitch_result_jpeg(self.h, pr, b, c, s), cap, _ref(params))

    def stitch_batch_result_jpeg(self, frame, shape, params=None, cap=None):
        """the JPEG of frame slot `frame` of the last stitch_step_batch; shape = (rows, cols) of that call"""
        rows, cols = shape
        return self._file_call(self.l.pf_jpeg_bound, cols, rows, lambda pr, b, c, s: self.l.pf_stitch_batch_result_jpeg(self.h, frame, pr, b, c, s), cap, _ref(params))

    # ---- TIFF files decoded on the device (pf_tiff_*): `data` = the file's bytes ----
    def tiff_set_inflate(self, on):
        """on: this context's tiff_decode* calls also take deflate files (pf_tiff_set_inflate; default off: they are refused)"""
        self._chk(self.l.pf_tiff_set_inflate(self.h, int(bool(on))))

    def tiff_decode(self, data, shape=None, row_step=None, out=None):
        """file bytes -> host BGRA (rows, cols, 4); shape = (rows, cols) the caller expects (default: the probe's).  row_step (bytes) or
        out (an array whose rows are row_step apart) selects a padded destination; the padding is left as it is"""
        buf = np.frombuffer(bytes(data), np.uint8)
        if shape is None:
            info = tiff_probe(data); shape = (info.rows, info.cols)
        rows, cols = shape
        step = int(row_step) if row_step is not None else cols * 4
        if out is None:
            out = np.empty((rows, step), np.uint8)
        self._chk(self.l.pf_tiff_decode(self.h, _p(buf), C.c_size_t(buf.size), cols, rows, _p(out), C.c_size_t(step)))
        return out[:, :cols * 4].reshape(rows, cols, 4)

    def tiff_decode_dev(self, data, cols, rows, d_out):
        buf = np.frombuffer(bytes(data), np.uint8)
        self._chk(self.l.pf_tiff_decode_dev(self.h, _p(buf), C.c_size_t(buf.size), cols, rows, C.c_void_p(d_out)))

    def tiff_decode_batch_dev(self, datas, cols, rows, d_outs):
        """n same-size files -> n device images"""
        n = len(datas)
        bufs = [np.frombuffer(bytes(d), np.uint8) for d in datas]
        files = (C.c_void_p * n)(*[b.ctypes.data for b in bufs]); sizes = (C.c_size_t * n)(*[b.size for b in bufs])
        self._chk(self.l.pf_tiff_decode_batch_dev(self.h, n, files, sizes, cols, rows, _dptrs(d_outs, n)))

    # ---- JPEG files decoded on the device (pf_jpeg_decode*): `data` = the file's bytes ----
    def jpeg_decode(self, data, shape=None, row_step=None, out=None):
        """file bytes -> host BGRA (rows, cols, 4); shape = (rows, cols) the caller expects (default: the probe's).  row_step (bytes) or
        out (an array whose rows are row_step apart) selects a padded destination; the padding is left as it is"""
        buf = np.frombuffer(bytes(data), np.uint8)
        if shape is None:
            info = jpeg_probe(data); shape = (info.rows, info.cols)
        rows, cols = shape
        step = int(row_step) if row_step is not None else cols * 4
        if out is None:
            out = np.empty((rows, step), np.uint8)
        self._chk(self.l.pf_jpeg_decode(self.h, _p(buf), C.c_size_t(buf.size), cols, rows, _p(out), C.c_size_t(step)))
        return out[:, :cols * 4].reshape(rows, cols, 4)

    def jpeg_decode_dev(self, data, cols, rows, d_out):
        buf = np.frombuffer(bytes(data), np.uint8)
        self._chk(self.l.pf_jpeg_decode_dev(self.h, _p(buf), C.c_size_t(buf.size), cols, rows, C.c_void_p(d_out)))

    def jpeg_decode_batch_dev(self, datas, cols, rows, d_outs):
        """n same-size files -> n device images"""
        n = len(datas)
        bufs = [np.frombuffer(bytes(d), np.uint8) for d in datas]
        files = (C.c_void_p * n)(*[b.ctypes.data for b in bufs]); sizes = (C.c_size_t * n)(*[b.size for b in bufs])
        self._chk(self.l.pf_jpeg_decode_batch_dev(self.h, n, files, sizes, cols, rows, _dptrs(d_outs, n)))

    def stage_jpeg_decode(self, data, nsub, nblocks, plane_bytes):
        """pf_stage_jpeg_decode: -> (states (nsub, 4) uint32, coef (nblocks, 64) int16, planes (plane_bytes,) uint8, counts (5,) int32:
        subsequences, rounds, launches, subsequence size, subsequences that changed after their first walk).  The caller gives the sizes (from the header's geometry)"""
        buf = np.frombuffer(bytes(data), np.uint8)
        states = np.zeros((nsub, 4), np.uint32); coef = np.zeros((nblocks, 64), np.int16); planes = np.zeros(plane_bytes, np.uint8)
        counts = np.zeros(5, np.int32)
        self._chk(self.l.pf_stage_jpeg_decode(self.h, _p(buf), C.c_size_t(buf.size), _p(states), C.c_size_t(states.nbytes), _p(coef), C.c_size_t(coef.nbytes),
                                              _p(planes), C.c_size_t(planes.nbytes), _p(counts)))
        return states, coef, planes, counts

    # ---- resize on the device (pf_resize*): Pillow's Image.resize of an RGBA image, byte for byte; filter = one of RESIZE_* ----
    def resize(self, image, out_cols, out_rows, filter=RESIZE_LANCZOS, out=None):
        """host BGRA (rows, cols, 4) array, any row stride -> host (out_rows, out_cols, 4); out: a destination array (its row stride is kept)"""
        a, cols, rows, step = _bgra(image)
        out, ostep = _dst(out, out_cols, out_rows)
        self._chk(self.l.pf_resize(self.h, _p(a), step, cols, rows, _p(out), ostep, out_cols, out_rows, int(filter)))
        return out

    def resize_dev(self, d_src, cols, rows, d_dst, out_cols, out_rows, filter=RESIZE_LANCZOS):
        self._chk(self.l.pf_resize_dev(self.h, C.c_void_p(d_src), cols, rows, C.c_void_p(d_dst), out_cols, out_rows, int(filter)))

    def resize_batch_dev(self, d_srcs, cols, rows, d_dsts, out_cols, out_rows, filter=RESIZE_LANCZOS):
        """n same-size device images -> n device images of out_cols x out_rows, one drain"""
        n = len(d_srcs)
        self._chk(self.l.pf_resize_batch_dev(self.h, n, _dptrs(d_srcs), cols, rows, _dptrs(d_dsts, n), out_cols, out_rows, int(filter)))

    def stitch_result_resized_dev(self, out_cols, out_rows, d_dst, filter=RESIZE_LANCZOS):
        """the composite the last stitch_step left in HBM, resized into d_dst (out_cols * out_rows * 4 bytes of device memory)"""
        self._chk(self.l.pf_stitch_result_resized_dev(self.h, out_cols, out_rows, int(filter), C.c_void_p(d_dst)))

    def stitch_batch_result_resized_dev(self, frame, out_cols, out_rows, d_dst, filter=RESIZE_LANCZOS):
        """frame slot `frame` of the last stitch_step_batch, resized into d_dst"""
        self._chk(self.l.pf_stitch_batch_result_resized_dev(self.h, frame, out_cols, out_rows, int(filter), C.c_void_p(d_dst)))

    def stage_resize_pass(self, image, axis, n_out, filter, premul, unpremul):
        """one pass of the resize alone (axis 0: k_resize_h to n_out columns, 1: k_resize_v to n_out rows) with its two fusions as given"""
        a = np.ascontiguousarray(image, dtype=np.uint8); rows, cols, _ = a.shape
        out = np.empty((max(n_out, 0), cols, 4) if axis else (rows, max(n_out, 0), 4), np.uint8)
        self._chk(self.l.pf_stage_resize_pass(self.h, _p(a), cols, rows, int(axis), int(n_out), int(filter), int(premul), int(unpremul), _p(out)))
        return out

    # ---- reprojection on the device (pf_reproject*): params = a ReprojectParams (reproject_params()) ----
    def reproject(self, image, out_cols, out_rows, params, out=None):
        """host BGRA (rows, cols, 4) equirectangular sphere, any row stride -> host (out_rows, out_cols, 4); out: a destination array (its row stride is kept)"""
        a, cols, rows, step = _bgra(image)
        out, ostep = _dst(out, out_cols, out_rows)
        self._chk(self.l.pf_reproject(self.h, _p(a), step, cols, rows, _p(out), ostep, out_cols, out_rows, C.byref(params)))
        return out

    def reproject_dev(self, d_src, cols, rows, d_dst, out_cols, out_rows, params):
        self._chk(self.l.pf_reproject_dev(self.h, C.c_void_p(d_src), cols, rows, C.c_void_p(d_dst), out_cols, out_rows, C.byref(params)))

    def reproject_batch_dev(self, d_srcs, cols, rows, d_dsts, out_cols, out_rows, params):
        """n same-size device images -> n device images of out_cols x out_rows, one drain"""
        n = len(d_srcs)
        self._chk(self.l.pf_reproject_batch_dev(self.h, n, _dptrs(d_srcs), cols, rows, _dptrs(d_dsts, n), out_cols, out_rows, C.byref(params)))

    def reproject_cube_dev(self, d_src, cols, rows, d_faces, face_size, params):
        """one device sphere -> six device faces of face_size x face_size (FACE_* order), one launch"""
        dsts = (C.c_void_p * 6)(*[C.c_void_p(int(x)) for x in d_faces])
        self._chk(self.l.pf_reproject_cube_dev(self.h, C.c_void_p(d_src), cols, rows, dsts, face_size, C.byref(params)))

    def stitch_result_reprojected_dev(self, out_cols, out_rows, params, d_dst):
        """the composite the last stitch_step left in HBM, reprojected into d_dst (out_cols * out_rows * 4 bytes of device memory)"""
        self._chk(self.l.pf_stitch_result_reprojected_dev(self.h, out_cols, out_rows, C.byref(params), C.c_void_p(d_dst)))

    def stitch_batch_result_reprojected_dev(self, frame, out_cols, out_rows, params, d_dst):
        """frame slot `frame` of the last stitch_step_batch, reprojected into d_dst"""
        self._chk(self.l.pf_stitch_batch_result_reprojected_dev(self.h, frame, out_cols, out_rows, C.byref(params), C.c_void_p(d_dst)))

    def stage_reproject_coords(self, cols, rows, out_cols, out_rows, params):
        """(fx, fy): the device's quantised source coordinates of every output pixel, int32 (out_rows, out_cols)"""
        fx = np.empty((out_rows, out_cols), np.int32); fy = np.empty((out_rows, out_cols), np.int32)
        self._chk(self.l.pf_stage_reproject_coords(self.h, cols, rows, out_cols, out_rows, C.byref(params), _p(fx), _p(fy)))
        return fx, fy

    # ---- lens remap on the device (pf_lens_*): lens = a Lens (lens()) ----
    def lens_remap(self, photo, cols, rows, lens, out=None):
        """host BGRA photo (photo_rows, photo_cols, 4), any row stride -> host canvas (rows, cols, 4); out: a destination array (its row stride is kept)"""
        a, photo_cols, photo_rows, step = _bgra(photo)
        out, ostep = _dst(out, cols, rows)
        self._chk(self.l.pf_lens_remap(self.h, _p(a), step, photo_cols, photo_rows, _p(out), ostep, cols, rows, C.byref(lens)))
        return out

    def lens_remap_dev(self, d_photo, photo_cols, photo_rows, d_canvas, cols, rows, lens):
        self._chk(self.l.pf_lens_remap_dev(self.h, C.c_void_p(d_photo), photo_cols, photo_rows, C.c_void_p(d_canvas), cols, rows, C.byref(lens)))

    def lens_remap_batch_dev(self, d_photos, photo_cols, photo_rows, d_canvases, cols, rows, lenses):
        """n same-size device photos -> n device canvases of cols x rows, image k under lenses[k], one drain"""
        n = len(d_photos)
        self._chk(self.l.pf_lens_remap_batch_dev(self.h, n, _dptrs(d_photos), photo_cols, photo_rows, _dptrs(d_canvases, n), cols, rows, (Lens * n)(*lenses)))

    def stage_lens_coords(self, photo_cols, photo_rows, cols, rows, lens):
        """(fx, fy): the device's quantised photo coordinates of every canvas pixel, int32 (rows, cols)"""
        fx = np.empty((rows, cols), np.int32); fy = np.empty((rows, cols), np.int32)
        self._chk(self.l.pf_stage_lens_coords(self.h, photo_cols, photo_rows, cols, rows, C.byref(lens), _p(fx), _p(fy)))
        return fx, fy

    # ---- device-resident entry points (raw device pointers as ints) ----
    def dev_alloc(self, nbytes):
        p = self.l.pf_dev_alloc(self.h, C.c_size_t(nbytes))
        if not p:
            raise PanoflowError(self.l.pf_last_error(self.h).decode())
        return p

    def selftest_packed_chains(self):
        """0 = the sweep's asm-block packed-fp32 chains give the compiler-scheduled forms' bits on this device"""
        self.l.pf_selftest_packed_chains.argtypes = [C.c_void_p]
        r = self.l.pf_selftest_packed_chains(self.h)
        if r < 0:
            self._chk(r)
        return r

    def dev_free(self, p):
        self.l.pf_dev_free(self.h, C.c_void_p(p))

    def host_array(self, shape, dtype=np.uint8):
        """numpy array over page-locked host memory (pf_host_alloc); freed with the context (keep the context alive while it is used)"""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = self.l.pf_host_alloc(self.h, C.c_size_t(nbytes))
        if not p:
            raise PanoflowError(self.l.pf_last_error(self.h).decode())
        self._pinned = getattr(self, "_pinned", []) + [p]
        buf = (C.c_uint8 * nbytes).from_address(p)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    def upload(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        self._chk(self.l.pf_upload(self.h, C.c_void_p(dptr), _p(arr), C.c_size_t(arr.nbytes)))

    def checksum_dev(self, dptr, nbytes):
        h = C.c_uint64(0)
        self._chk(self.l.pf_checksum_dev(self.h, C.c_void_p(dptr), C.c_size_t(nbytes), C.byref(h)))
        return h.value

    def download(self, arr, dptr):
        self._chk(self.l.pf_download(self.h, _p(arr), C.c_void_p(dptr), C.c_size_t(arr.nbytes)))
        return arr

    def novel_view_dev(self, d_l, d_r, cols, rows, max_pct, d_blend, d_out, d_f0=None, d_f1=None):
        self._chk(self.l.pf_novel_view_dev(self.h, C.c_void_p(d_l), C.c_void_p(d_r), cols, rows, max_pct, C.c_void_p(d_blend), C.c_void_p(d_out),
                                           C.c_void_p(d_f0) if d_f0 else None, C.c_void_p(d_f1) if d_f1 else None))

    def novel_view_batch_dev(self, d_l, d_r, cols, rows, max_pct, d_blend, d_out, d_f0=None, d_f1=None, in_flight=4):
        """throughput mode: lists of device pointers, `in_flight` pairs side by side on this GPU"""
        n = len(d_l)
        arr = lambda v: (C.c_void_p * n)(*[C.c_void_p(int(x)) if x else None for x in v])
        self._chk(self.l.pf_novel_view_batch_dev(self.h, n, arr(d_l), arr(d_r), cols, rows, max_pct, arr(d_blend), arr(d_out),
                                                 arr(d_f0) if d_f0 else None, arr(d_f1) if d_f1 else None, in_flight))

    def flow_bidir_dev(self, d_l, d_r, cols, rows, max_pct, d_f0, d_f1):
        self._chk(self.l.pf_flow_bidir_dev(self.h, C.c_void_p(d_l), C.c_void_p(d_r), cols, rows, max_pct, C.c_void_p(d_f0), C.c_void_p(d_f1)))

    def blend_dev(self, d_l, d_r, d_f0, d_f1, d_blend, cols, rows, d_out):
        self._chk(self.l.pf_blend_dev(self.h, C.c_void_p(d_l), C.c_void_p(d_r), C.c_void_p(d_f0), C.c_void_p(d_f1), C.c_void_p(d_blend), cols, rows,
                                      C.c_void_p(d_out)))

    # ---- stage-level entry points ----
    def stage_preprocess(self, bgra, pad=0):
        a = _u8(bgra); rows, cols, _ = a.shape
        dw = int(np.float32(cols + 2 * pad) * np.float32(0.5)); dh = int(np.float32(rows) * np.float32(0.5))
        g = np.empty((dh, dw), np.float32); al = np.empty((dh, dw), np.float32)
        self._chk(self.l.pf_stage_preprocess(self.h, _p(a), cols, rows, pad, _p(g), _p(al)))
        return g, al

    def stage_pyr_down(self, src, dw, dh):
        s = _f32(src); sh, sw = s.shape
        d = np.empty((dh, dw), np.float32)
        self._chk(self.l.pf_stage_pyr_down(self.h, _p(s), sw, sh, _p(d), dw, dh))
        return d

    def stage_gradients(self, img):
        s = _f32(img); h, w = s.shape
        g = np.empty((h, w, 2), np.float32)
        self._chk(self.l.pf_stage_gradients(self.h, _p(s), w, h, _p(g)))
        return g

    def stage_gauss(self, src, ksize, sigma):
        s = _f32(src)
        h, w = s.shape[:2]; cn = 1 if s.ndim == 2 else s.shape[2]
        d = np.empty_like(s)
        self._chk(self.l.pf_stage_gauss(self.h, _p(s), w, h, cn, ksize, C.c_double(sigma), _p(d)))
        return d

    def stage_median5(self, flow):
        s = _f32(flow); h, w, _ = s.shape
        d = np.empty_like(s)
        self._chk(self.l.pf_stage_median5(self.h, _p(s), w, h, _p(d)))
        return d

    def stage_sweep(self, g0, g1, blurred, a0, a1, flow, forward):
        f = _f32(flow).copy(); h, w, _ = f.shape
        self._chk(self.l.pf_stage_sweep(self.h, _p(_f32(g0)), _p(_f32(g1)), _p(_f32(blurred)), _p(_f32(a0)), _p(_f32(a1)), _p(f), w, h, int(forward)))
        return f

    def stage_diffusion(self, a0, a1, flow):
        f = _f32(flow).copy(); h, w, _ = f.shape
        self._chk(self.l.pf_stage_diffusion(self.h, _p(_f32(a0)), _p(_f32(a1)), _p(f), w, h))
        return f

    def stage_upsample_cubic(self, flow, dw, dh, scale):
        s = _f32(flow); sh, sw, _ = s.shape
        d = np.empty((dh, dw, 2), np.float32)
        self._chk(self.l.pf_stage_upsample_cubic(self.h, _p(s), sw, sh, _p(d), dw, dh, C.c_float(scale)))
        return d

    def stage_final(self, flow, pad_cols, rows, pad, scale):
        s = _f32(flow); sh, sw, _ = s.shape
        d = np.empty((rows, pad_cols - 2 * pad, 2), np.float32)
        self._chk(self.l.pf_stage_final(self.h, _p(s), sw, sh, pad_cols, rows, pad, C.c_float(scale), _p(d)))
        return d

    def stage_adjust_initial_flow(self, i0, i1, a0, a1, hint, max_pct):
        s = _f32(i0); h, w = s.shape
        f = np.empty((h, w, 2), np.float32)
        self._chk(self.l.pf_stage_adjust_initial_flow(self.h, _p(s), _p(_f32(i1)), _p(_f32(a0)), _p(_f32(a1)), w, h, hint, max_pct, _p(f)))
        return f

    def stage_level(self, i0, i1, a0, a1, flow_in, hint, max_pct):
        s = _f32(i0); h, w = s.shape
        f = np.empty((h, w, 2), np.float32)
        fin = None if flow_in is None else _f32(flow_in)
        self._chk(self.l.pf_stage_level(self.h, _p(s), _p(_f32(i1)), _p(_f32(a0)), _p(_f32(a1)), w, h, None if fin is None else _p(fin), hint, max_pct, _p(f)))
        return f

    def stage_blend_smooth(self, blend, md):
        b = _f32(blend).copy(); rows, cols = b.shape
        self._chk(self.l.pf_stage_blend_smooth(self.h, _p(b), _p(_f32(md)), cols, rows))
        return b

    def stage_tile_blur(self, blend, md, step, k, form=-1):
        """the tile pass of the ramp smoothing alone, explicit geometry; form -1 = the library's choice, 0 = resident, 1 = streamed"""
        b = _f32(blend).copy(); rows, cols = b.shape
        m = _f32(md)
        if m.shape != b.shape:
            raise ValueError("blend and merged_dis differ in shape")
        self._chk(self.l.pf_stage_tile_blur(self.h, _p(b), _p(m), cols, rows, int(step), int(k), int(form)))
        return b

    def stage_box_blur(self, src, k):
        """the final box blur of the ramp smoothing alone with an explicit kernel width: src (rows, cols), or (n, rows, cols) for a batch
        of 1..3 planes; returns the blurred planes in the input's shape"""
        s = _f32(src); lone = s.ndim == 2
        if lone:
            s = s[None]
        n, rows, cols = s.shape
        d = np.empty_like(s)
        self._chk(self.l.pf_stage_box_blur(self.h, n, _p(s), cols, rows, int(k), _p(d)))
        return d[0] if lone else d

    def stage_gauss15_form(self, form, src, a0=None, a1=None, size=None, mul=1.0, max_blocks=0):
        """One form of the fused Gaussian 15 ("plain", "mix", "ups", "med_mix") on a batch of planes: src (n, h, w, 2), or (h, w, 2) for a lone
        plane; the MIX forms take alphas of shape src.shape[:-1]; "ups" takes the coarse planes as src and size=(w, h) of the result.
        Returns dst, or (dst, up) for "ups", shaped like the input batch."""
        fid = {"plain": 0, "mix": 1, "ups": 2, "med_mix": 3}[form]
        s = _f32(src); lone = s.ndim == 3
        if lone:
            s = s[None]
        n, sh, sw, _ = s.shape
        w, h = size if fid == 2 else (sw, sh)
        al = [None, None]
        if fid in (1, 3):
            al = [_f32(a)[None] if lone else _f32(a) for a in (a0, a1)]
            assert al[0].shape == (n, h, w) and al[1].shape == (n, h, w)
        dst = np.empty((n, h, w, 2), np.float32); up = np.empty((n, h, w, 2), np.float32) if fid == 2 else None
        self._chk(self.l.pf_stage_gauss15_form(self.h, fid, n, int(max_blocks), _p(s), sw, sh, C.c_float(mul), None if al[0] is None else _p(al[0]),
                                               None if al[1] is None else _p(al[1]), w, h, _p(dst), None if up is None else _p(up)))
        if lone:
            dst = dst[0]; up = None if up is None else up[0]
        return (dst, up) if fid == 2 else dst

    def stage_level_table(self, sizes, img0, img1, a0, a1, first=0, total=0, max_blocks=0):
        """Gradients and gate + boxes + count of a whole level table.  sizes: [(w, h), ...]; img0 / img1 / a0 / a1: per pair a list of
        (h, w) planes, one per level (a lone pair may pass the list itself instead of a list of lists).  Returns a dict: off (level
        offsets in the padded plane + its size P), g0 / g1 (n, P, 2) float32 and gate (n, P) uint8 as whole padded planes (unwritten = 0xFF
        bytes), boxes (n, levels, 4), count0 (n,)."""
        nl = len(sizes)
        if nl and isinstance(img0[0], np.ndarray) and img0[0].ndim == 2:
            img0, img1, a0, a1 = [img0], [img1], [a0], [a1]
        n = len(img0)

        def pack(planes):
            for pair in planes:
                assert len(pair) == nl and all(pl.shape == (hh, ww) for pl, (ww, hh) in zip(pair, sizes))
            return np.ascontiguousarray(np.concatenate([_f32(pl).ravel() for pair in planes for pl in pair]))
        ws = (C.c_int * nl)(*[int(s[0]) for s in sizes]); hs = (C.c_int * nl)(*[int(s[1]) for s in sizes])
        P = sum((int(w) * int(h) + 63) & ~63 for w, h in sizes)
        off = np.zeros(nl + 1, np.int64)
        g0 = np.empty((n, P, 2), np.float32); g1 = np.empty((n, P, 2), np.float32); gate = np.empty((n, P), np.uint8)
        boxes = np.empty((n, nl, 4), np.int32); cnt = np.empty(n, np.int32)
        pk = [pack(v) for v in (img0, img1, a0, a1)]
        self._chk(self.l.pf_stage_level_table(self.h, nl, ws, hs, n, _p(pk[0]), _p(pk[1]), _p(pk[2]), _p(pk[3]), C.c_longlong(int(first)), C.c_longlong(int(total)),
                                              int(max_blocks), _p(off), _p(g0), _p(g1), _p(gate), _p(boxes), _p(cnt)))
        assert int(off[nl]) == P
        return {"off": off, "g0": g0, "g1": g1, "gate": gate, "boxes": boxes, "count0": cnt}

    def stage_preprocess_batch(self, images, pad=0):
        """1..3 BGRA images of one size, (n, rows, cols, 4), each in a device buffer of its own, through the batched form of the downscale and
        the pre-blur (one image: the lone form).  Returns gray, alpha as (n, padded) float32: each pair's w0 * h0 plane and the padding behind
        it inside the slab (unwritten = 0xFF bytes), and (w0, h0)."""
        a = _u8(images); n, rows, cols, _ = a.shape
        dw = int(np.float32(cols + 2 * pad) * np.float32(0.5)); dh = int(np.float32(rows) * np.float32(0.5))
        npad = (max(dw * dh, 0) + 63) & ~63
        g = np.empty((n, npad), np.float32); al = np.empty((n, npad), np.float32)
        self._chk(self.l.pf_stage_preprocess_batch(self.h, n, _p(a), cols, rows, int(pad), _p(g), _p(al)))
        return g, al, (dw, dh)

    def stage_pyramid(self, level0, mode=1):
        """The solver's pyramid loop on 1..3 pairs.  level0: (n, 4, h0, w0) = I0, I1, alpha0, alpha1 of each pair.  mode 0 = one level per
        launch, 1 = the product's rule, 2 / 3 = that many levels per launch wherever that many are left.  Returns a dict: sizes [(w, h)],
        off (level offsets + the plane size P), ks (levels written per launch), planes (n, 4, P) float32 whole padded planes."""
        s = _f32(level0); n, four, h0, w0 = s.shape
        assert four == 4
        cap_l = 128; cap_p = 6 * w0 * h0 + 64 * cap_l   # a 0.9x pyramid holds 1 / (1 - 0.81) = 5.3 times level 0, plus 64 elements of padding per level
        ws = (C.c_int * cap_l)(); hs = (C.c_int * cap_l)(); ks = (C.c_int * cap_l)(); nlev = C.c_int(0); nk = C.c_int(0)
        off = np.zeros(cap_l + 1, np.int64)
        buf = np.empty(n * 4 * cap_p, np.float32)
        self._chk(self.l.pf_stage_pyramid(self.h, n, int(mode), _p(s), w0, h0, cap_l, C.c_longlong(cap_p), C.byref(nlev), ws, hs, _p(off), ks, C.byref(nk), _p(buf)))
        nl = nlev.value; P = int(off[nl])
        return {"sizes": [(ws[i], hs[i]) for i in range(nl)], "off": off[:nl + 1].copy(), "ks": [ks[i] for i in range(nk.value)],
                "planes": buf[:n * 4 * P].reshape(n, 4, P).copy()}

    def stage_adjust_initial_flow_batch(self, i0, i1, a0, a1, hint, max_pct):
        """The coarsest-level search on 1..3 pairs of one level size in slabs, (n, h, w) each.  Returns (n, padded) float32: each pair's
        h x w x 2 flow plane and the padding behind it (unwritten = 0xFF bytes)."""
        s = [_f32(v) for v in (i0, i1, a0, a1)]; n, h, w = s[0].shape
        assert all(v.shape == (n, h, w) for v in s)
        f = np.empty((n, (2 * w * h + 63) & ~63), np.float32)
        self._chk(self.l.pf_stage_adjust_initial_flow_batch(self.h, n, _p(s[0]), _p(s[1]), _p(s[2]), _p(s[3]), w, h, int(hint), int(max_pct), _p(f)))
        return f

    def stage_intensity_ratio(self, i0, i1, a0, a1):
        """k_intensity_ratio on 1..3 pairs of n elements, (pairs, n) each; returns (pairs,) float32"""
        s = [_f32(v) for v in (i0, i1, a0, a1)]; m, n = s[0].shape
        assert all(v.shape == (m, n) for v in s)
        r = np.empty(m, np.float32)
        self._chk(self.l.pf_stage_intensity_ratio(self.h, m, _p(s[0]), _p(s[1]), _p(s[2]), _p(s[3]), n, _p(r)))
        return r

    def set_solver_params(self, **kw):
        """PixFlow's constructor arguments for every later solve on this context (pf_set_solver_params); no arguments = the factory's presets.
        Keys: pyr_scale_factor, smoothness_coef, vertical_regularization_coef, horizontal_regularization_coef, gradient_step_size, downscale_factor."""
        p = SolverParams()
        self.l.pf_solver_params_init(C.byref(p))
        for k, v in kw.items():
            if not hasattr(p, k):
                raise PanoflowError("unknown solver parameter %r" % k)
            setattr(p, k, v)
        self._chk(self.l.pf_set_solver_params(self.h, C.byref(p)))

    def solver_params(self):
        p = SolverParams()
        self._chk(self.l.pf_get_solver_params(self.h, C.byref(p)))
        return {k: getattr(p, k) for k, _ in SolverParams._fields_}

    def last_swept_steps(self):
        """dependent wavefront steps of one direction of the last solve (windows of gated pixels)"""
        return int(self.l.pf_last_swept_steps(self.h))

    def last_warning(self):
        """(text of the last performance warning raised on this context or "", how many were raised)  -- include/panoflow.h"""
        return self.l.pf_last_warning(self.h).decode(), int(self.l.pf_warning_count(self.h))

    # ---- profiling ----
    def profile_enable(self, on=True):
        """0/False off, 1/True every kernel family, 2 only the sweep kernels."""
        self.l.pf_profile_enable(self.h, int(on))

    def profile_reset(self):
        self.l.pf_profile_reset(self.h)

    def profile(self):
        out = {}
        for i in range(self.l.pf_profile_count(self.h)):
            name = C.create_string_buffer(64); ms = C.c_double(0); n = C.c_int(0)
            self.l.pf_profile_get(self.h, i, name, 64, C.byref(ms), C.byref(n))
            out[name.value.decode()] = (ms.value, n.value)
        return out
