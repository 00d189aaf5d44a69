"""ctypes binding of libndt_hip.so (include/ndt_hip.h) -- the product's only compute path.

There is deliberately no fallback: if the shared library is missing or no MI355X is present,
construction raises.  The CPU restatement under oracle/ is test infrastructure and is never
imported from here.
"""
import ctypes as C
import os

import numpy as np

from .flat_scene import NDT_E_STATE, RenderParams, RenderStats, shard_rows

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NDT_HIP_LIB") or os.path.join(_HERE, "libndt_hip.so")

# every entry point include/ndt_hip.h declares
API_SYMBOLS = [
    "ndt_hip_create", "ndt_hip_destroy", "ndt_hip_upload_scene", "ndt_hip_render_device", "ndt_hip_render",
    "ndt_hip_trace_rays", "ndt_hip_quantize_device", "ndt_hip_shard_rows", "ndt_hip_stream",
    "ndt_hip_synchronize", "ndt_hip_last_error", "ndt_hip_abi_version", "ndt_hip_hcube_hull_box", "ndt_hip_hcube_face_boxes", "ndt_hip_hcube_face_boxes_all", "ndt_hip_hcube_face_tree", "ndt_hip_hcube_face_groups",
    "ndt_hip_render_depth_device", "ndt_hip_render_depth", "ndt_hip_render_rgba8", "ndt_hip_render_multi_device",
    "ndt_hip_render_multi", "ndt_hip_device_count", "ndt_hip_device", "ndt_hip_set_option", "ndt_hip_multi_path_taken",
    "ndt_hip_item_boxes", "ndt_hip_check_scene", "ndt_hip_render_rgba8_async", "ndt_hip_render_rgba8_wait",
    "ndt_hip_fit_spheres", "ndt_hip_fit_launches",
    "ndt_hip_build_kdtree", "ndt_hip_kdtree_fetch", "ndt_hip_kd_launches",
    "ndt_hip_png_bound", "ndt_hip_encode_png_device", "ndt_hip_encode_png", "ndt_hip_render_png",
    "ndt_hip_jpeg_bound", "ndt_hip_encode_jpeg_device", "ndt_hip_encode_jpeg", "ndt_hip_render_jpeg",
    "ndt_hip_depth_rgba8_device", "ndt_hip_render_rgba8_depth", "ndt_hip_render_png_depth", "ndt_hip_depth_launches", "ndt_hip_depth_ms",
    "ndt_hip_ssaa_fold_device", "ndt_hip_render_ssaa_device", "ndt_hip_render_ssaa", "ndt_hip_render_ssaa_rgba8", "ndt_hip_render_ssaa_png",
    "ndt_hip_render_ssaa_jpeg", "ndt_hip_render_ssaa_rgba8_depth", "ndt_hip_ssaa_launches", "ndt_hip_ssaa_ms",
    "ndt_hip_quantize16_device", "ndt_hip_depth_grey16_device", "ndt_hip_png16_bound", "ndt_hip_encode_png16_device", "ndt_hip_encode_png16",
    "ndt_hip_render_png16", "ndt_hip_render_png16_depth", "ndt_hip_render_ssaa_png16", "ndt_hip_render_ssaa_png16_depth",
    "ndt_hip_apng_bound", "ndt_hip_apng_begin", "ndt_hip_apng_add_device", "ndt_hip_apng_add", "ndt_hip_render_apng_frame", "ndt_hip_apng_end",
    "ndt_hip_exr_bound", "ndt_hip_encode_exr_device", "ndt_hip_encode_exr", "ndt_hip_render_exr", "ndt_hip_render_ssaa_exr",
    "ndt_hip_render_features", "ndt_hip_render_features_device", "ndt_hip_features_launches", "ndt_hip_exr_features_bound",
    "ndt_hip_encode_exr_features_device", "ndt_hip_render_exr_features", "ndt_hip_render_ssaa_exr_features",
    "ndt_hip_denoise_device", "ndt_hip_render_denoised_device", "ndt_hip_render_denoised", "ndt_hip_render_denoised_rgba8",
    "ndt_hip_render_denoised_png", "ndt_hip_render_denoised_jpeg", "ndt_hip_render_denoised_exr", "ndt_hip_denoise_launches", "ndt_hip_denoise_ms",
    "ndt_hip_render_moments_device", "ndt_hip_render_moments", "ndt_hip_sample_variance_device", "ndt_hip_vdenoise_device",
    "ndt_hip_render_vdenoised_device", "ndt_hip_render_vdenoised", "ndt_hip_render_vdenoised_rgba8", "ndt_hip_render_vdenoised_png",
    "ndt_hip_render_vdenoised_jpeg", "ndt_hip_render_vdenoised_exr",
    "ndt_hip_ao_device", "ndt_hip_render_ao_device", "ndt_hip_render_ao", "ndt_hip_ao_apply_device", "ndt_hip_render_ao_shaded_device",
    "ndt_hip_render_ao_shaded", "ndt_hip_render_ao_shaded_rgba8", "ndt_hip_render_ao_shaded_png", "ndt_hip_render_ao_shaded_jpeg",
    "ndt_hip_exr_ao_bound", "ndt_hip_encode_exr_ao_device", "ndt_hip_render_exr_ao", "ndt_hip_ao_launches", "ndt_hip_ao_ms",
]

IMAGE_F64, IMAGE_RGBA8 = 0, 1      # enum ndt_image_format
MULTI_NONE, MULTI_LOCAL, MULTI_PEER, MULTI_STAGED = 0, 1, 2, 3     # enum ndt_multi_path


class NdtHipError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("libndt_hip error %d: %s" % (code, message))
        self.code = code


_lib = None


def load_library():
    """Load libndt_hip.so (built in-tree by __graft_entry__.build() / ndt_amd/csrc/Makefile)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            "%s is missing: build it with `make -C ndt_amd/csrc` (or __graft_entry__.build()). "
            "ndt_amd has no CPU fallback." % LIB_PATH)
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64.so.7 +
    # libhsa-runtime64.so, and a process that loads /opt/rocm's copy first and torch's second
    # ends up with two HSA runtimes ("No HIP GPUs are available").  Importing torch first makes
    # the dynamic loader resolve our NEEDED libamdhip64.so.7 to the copy torch already mapped.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    lib.ndt_hip_last_error.restype = C.c_char_p
    lib.ndt_hip_stream.restype = C.c_void_p
    lib.ndt_hip_stream.argtypes = [C.c_void_p]
    lib.ndt_hip_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.ndt_hip_destroy.argtypes = [C.c_void_p]
    lib.ndt_hip_upload_scene.argtypes = [C.c_void_p, C.c_void_p]
    lib.ndt_hip_render_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ndt_hip_render.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ndt_hip_render_depth_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ndt_hip_render_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ndt_hip_trace_rays.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 6
    lib.ndt_hip_quantize_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.ndt_hip_synchronize.argtypes = [C.c_void_p]
    lib.ndt_hip_shard_rows.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    lib.ndt_hip_hcube_hull_box.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.ndt_hip_hcube_face_boxes.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.ndt_hip_hcube_face_boxes_all.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
    lib.ndt_hip_hcube_face_boxes_all.restype = C.c_int64
    if hasattr(lib, "ndt_hip_hcube_face_groups"):
        lib.ndt_hip_hcube_face_groups.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.ndt_hip_hcube_face_groups.restype = C.c_int
    if hasattr(lib, "ndt_hip_hcube_face_tree"):     # (absent from round 3's library, which profiles/ab_libs.sh still loads to compare builds)
        lib.ndt_hip_hcube_face_tree.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.ndt_hip_hcube_face_tree.restype = C.c_int64
    lib.ndt_hip_render_rgba8.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ndt_hip_render_multi.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.ndt_hip_render_multi_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.ndt_hip_device.argtypes = [C.c_void_p]
    lib.ndt_hip_multi_path_taken.argtypes = [C.c_void_p]
    lib.ndt_hip_item_boxes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "ndt_hip_check_scene"):         # (absent from earlier builds, which profiles/ab_libs.sh loads to compare)
        lib.ndt_hip_check_scene.argtypes = [C.c_void_p]
    lib.ndt_hip_render_rgba8_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ndt_hip_render_rgba8_wait.argtypes = [C.c_void_p]
    lib.ndt_hip_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    if hasattr(lib, "ndt_hip_fit_spheres"):         # (absent from earlier builds, which profiles/ab_libs.sh loads to compare)
        lib.ndt_hip_fit_spheres.argtypes = [C.c_void_p, C.c_int32, C.c_int64] + [C.c_void_p] * 5
        lib.ndt_hip_fit_launches.argtypes = [C.c_void_p]
    if hasattr(lib, "ndt_hip_build_kdtree"):
        lib.ndt_hip_build_kdtree.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 4
        lib.ndt_hip_kdtree_fetch.argtypes = [C.c_void_p] * 6
        lib.ndt_hip_kd_launches.argtypes = [C.c_void_p]
    if hasattr(lib, "ndt_hip_png_bound"):
        lib.ndt_hip_png_bound.argtypes = [C.c_int32, C.c_int32]
        lib.ndt_hip_png_bound.restype = C.c_int64
        lib.ndt_hip_encode_png_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
        lib.ndt_hip_encode_png.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
        lib.ndt_hip_render_png.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    if hasattr(lib, "ndt_hip_jpeg_bound"):
        lib.ndt_hip_jpeg_bound.argtypes = [C.c_int32, C.c_int32, C.c_void_p]
        lib.ndt_hip_jpeg_bound.restype = C.c_int64
        lib.ndt_hip_encode_jpeg_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        lib.ndt_hip_encode_jpeg.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        lib.ndt_hip_render_jpeg.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    if hasattr(lib, "ndt_hip_depth_rgba8_device"):
        lib.ndt_hip_depth_rgba8_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        lib.ndt_hip_render_rgba8_depth.argtypes = [C.c_void_p] * 6
        lib.ndt_hip_render_png_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]
        lib.ndt_hip_depth_launches.argtypes = [C.c_void_p]
        lib.ndt_hip_depth_ms.argtypes = [C.c_void_p]
        lib.ndt_hip_depth_ms.restype = C.c_double
    if hasattr(lib, "ndt_hip_ssaa_fold_device"):    # (absent from earlier builds, which profiles/ab_libs.sh loads to compare)
        lib.ndt_hip_ssaa_fold_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        lib.ndt_hip_render_ssaa_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.ndt_hip_render_ssaa.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.ndt_hip_render_ssaa_rgba8.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        lib.ndt_hip_render_ssaa_png.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        lib.ndt_hip_render_ssaa_jpeg.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        lib.ndt_hip_render_ssaa_rgba8_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.ndt_hip_ssaa_launches.argtypes = [C.c_void_p]
        lib.ndt_hip_ssaa_ms.argtypes = [C.c_void_p]
        lib.ndt_hip_ssaa_ms.restype = C.c_double
    if hasattr(lib, "ndt_hip_png16_bound"):         # (absent from earlier builds, which profiles/ab_libs.sh loads to compare)
        lib.ndt_hip_quantize16_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        lib.ndt_hip_depth_grey16_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        lib.ndt_hip_png16_bound.argtypes = [C.c_int32, C.c_int32, C.c_int32]
        lib.ndt_hip_png16_bound.restype = C.c_int64
        lib.ndt_hip_encode_png16_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
        lib.ndt_hip_encode_png16.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
        lib.ndt_hip_render_png16.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        lib.ndt_hip_render_png16_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                   C.c_void_p]
        lib.ndt_hip_render_ssaa_png16.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        lib.ndt_hip_render_ssaa_png16_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                        C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "ndt_hip_apng_bound"):          # (absent from earlier builds, which profiles/ab_libs.sh loads to compare)
        lib.ndt_hip_apng_bound.argtypes = [C.c_int32, C.c_int32]
        lib.ndt_hip_apng_bound.restype = C.c_int64
        lib.ndt_hip_apng_begin.argtypes = [C.c_void_p] + [C.c_int32] * 6
        lib.ndt_hip_apng_add_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        lib.ndt_hip_apng_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        lib.ndt_hip_render_apng_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        lib.ndt_hip_apng_end.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    if hasattr(lib, "ndt_hip_exr_bound"):           # (absent from earlier builds, which profiles/ab_libs.sh loads to compare)
        lib.ndt_hip_exr_bound.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_int32]
        lib.ndt_hip_exr_bound.restype = C.c_int64
        lib.ndt_hip_encode_exr_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                                  C.c_void_p]
        lib.ndt_hip_encode_exr.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        lib.ndt_hip_render_exr.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        lib.ndt_hip_render_ssaa_exr.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                                C.c_void_p]
    if hasattr(lib, "ndt_hip_render_features"):     # (likewise)
        lib.ndt_hip_render_features.argtypes = [C.c_void_p] * 4
        lib.ndt_hip_render_features_device.argtypes = [C.c_void_p] * 4
        lib.ndt_hip_features_launches.argtypes = [C.c_void_p]
        lib.ndt_hip_exr_features_bound.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        lib.ndt_hip_exr_features_bound.restype = C.c_int64
        lib.ndt_hip_encode_exr_features_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                                           C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        lib.ndt_hip_render_exr_features.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64,
                                                    C.c_void_p, C.c_void_p]
        lib.ndt_hip_render_ssaa_exr_features.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                                         C.c_int64, C.c_void_p, C.c_void_p]
    if hasattr(lib, "ndt_hip_denoise_device"):      # (likewise)
        lib.ndt_hip_denoise_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        lib.ndt_hip_render_denoised_device.argtypes = [C.c_void_p] * 5
        lib.ndt_hip_render_denoised.argtypes = [C.c_void_p] * 5
        lib.ndt_hip_render_denoised_rgba8.argtypes = [C.c_void_p] * 5
        lib.ndt_hip_render_denoised_png.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        lib.ndt_hip_render_denoised_jpeg.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        lib.ndt_hip_render_denoised_exr.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        lib.ndt_hip_denoise_launches.argtypes = [C.c_void_p]
        lib.ndt_hip_denoise_ms.argtypes = [C.c_void_p]
        lib.ndt_hip_denoise_ms.restype = C.c_double
    if hasattr(lib, "ndt_hip_vdenoise_device"):     # (likewise)
        lib.ndt_hip_render_moments_device.argtypes = [C.c_void_p] * 6
        lib.ndt_hip_render_moments.argtypes = [C.c_void_p] * 6
        lib.ndt_hip_sample_variance_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        lib.ndt_hip_vdenoise_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                                C.c_void_p, C.c_void_p]
        lib.ndt_hip_render_vdenoised_device.argtypes = [C.c_void_p] * 5
        lib.ndt_hip_render_vdenoised.argtypes = [C.c_void_p] * 5
        lib.ndt_hip_render_vdenoised_rgba8.argtypes = [C.c_void_p] * 5
        lib.ndt_hip_render_vdenoised_png.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        lib.ndt_hip_render_vdenoised_jpeg.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        lib.ndt_hip_render_vdenoised_exr.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    if hasattr(lib, "ndt_hip_ao_device"):           # (likewise)
        lib.ndt_hip_ao_device.argtypes = [C.c_void_p] * 6
        lib.ndt_hip_render_ao_device.argtypes = [C.c_void_p] * 6
        lib.ndt_hip_render_ao.argtypes = [C.c_void_p] * 6
        lib.ndt_hip_ao_apply_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_void_p]
        lib.ndt_hip_render_ao_shaded_device.argtypes = [C.c_void_p] * 6
        lib.ndt_hip_render_ao_shaded.argtypes = [C.c_void_p] * 6
        lib.ndt_hip_render_ao_shaded_rgba8.argtypes = [C.c_void_p] * 5
        lib.ndt_hip_render_ao_shaded_png.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        lib.ndt_hip_render_ao_shaded_jpeg.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                      C.c_void_p]
        lib.ndt_hip_exr_ao_bound.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        lib.ndt_hip_exr_ao_bound.restype = C.c_int64
        lib.ndt_hip_encode_exr_ao_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                                     C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        lib.ndt_hip_render_exr_ao.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                              C.c_void_p, C.c_void_p]
        lib.ndt_hip_ao_launches.argtypes = [C.c_void_p]
        lib.ndt_hip_ao_ms.argtypes = [C.c_void_p]
        lib.ndt_hip_ao_ms.restype = C.c_double
    _lib = lib
    return lib


class KdCounts(C.Structure):
    """ndt_kd_counts: what ndt_hip_build_kdtree says about the tree it left in the context"""
    _fields_ = [("n_kd_nodes", C.c_int32), ("n_leaf_refs", C.c_int32), ("n_inf", C.c_int32), ("depth", C.c_int32),
                ("launches", C.c_int32), ("grows", C.c_int32)]


class PngStats(C.Structure):
    """ndt_png_stats: what the device encoder says about the file it made"""
    _fields_ = [("png_bytes", C.c_int64), ("idat_bytes", C.c_int64), ("chunks", C.c_int32), ("chunks_stored", C.c_int32),
                ("launches", C.c_int32), ("rows_filter", C.c_int32 * 3), ("encode_ms", C.c_double)]


class ApngStats(C.Structure):
    """ndt_apng_stats: what the device says about the frame it appended to the animated PNG"""
    _fields_ = [("bytes", C.c_int64), ("zlib_bytes", C.c_int64), ("changed", C.c_int64), ("translucent", C.c_int64),
                ("frame", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("blend", C.c_int32),
                ("launches", C.c_int32), ("reserved", C.c_int32), ("encode_ms", C.c_double)]


class JpegParams(C.Structure):
    """ndt_jpeg_params: quality 1 .. 100 (0 = 95), sampling 0 = 4:2:0 / 1 = 4:4:4"""
    _fields_ = [("quality", C.c_int32), ("sampling", C.c_int32), ("reserved", C.c_int32 * 2)]


class JpegStats(C.Structure):
    """ndt_jpeg_stats: what the device encoder says about the file it made"""
    _fields_ = [("jpeg_bytes", C.c_int64), ("scan_bytes", C.c_int64), ("stuffed_bytes", C.c_int64), ("mcus", C.c_int32),
                ("intervals", C.c_int32), ("launches", C.c_int32), ("passes_max", C.c_int32), ("encode_ms", C.c_double)]


class ExrParams(C.Structure):
    """ndt_exr_params: pixel_type of the colour channels, 1 half / 2 float (0 = half)"""
    _fields_ = [("pixel_type", C.c_int32), ("reserved", C.c_int32 * 3)]


class ExrStats(C.Structure):
    """ndt_exr_stats: what the device encoder says about the OpenEXR file it made"""
    _fields_ = [("file_bytes", C.c_int64), ("raw_bytes", C.c_int64), ("blocks", C.c_int32), ("blocks_raw", C.c_int32),
                ("launches", C.c_int32), ("pad", C.c_int32), ("ms", C.c_double)]


EXR_PIXEL = {"half": 1, "float": 2}


def exr_params(pixel="half"):
    """The ndt_exr_params of pixel "half" or "float"; ValueError for anything else."""
    if str(pixel) not in EXR_PIXEL:
        raise ValueError("EXR pixel %r is neither 'half' nor 'float'" % (pixel,))
    return ExrParams(EXR_PIXEL[str(pixel)])


def exr_bound(width, rows, pixel="half", depth_map=False):
    """ndt_hip_exr_bound: the largest OpenEXR file the device encoder can produce for a width x rows image (host arithmetic)."""
    ep = exr_params(pixel)
    n = int(load_library().ndt_hip_exr_bound(int(width), int(rows), C.byref(ep), 1 if depth_map else 0))
    if n < 0:
        raise ValueError("no EXR of %d x %d: the size is empty or its samples exceed 2^31 - 1 bytes" % (width, rows))
    return n


FEATURES = {"id": 1, "position": 2, "normal": 4}        # NDT_FEATURE_*


class FeaturePlanes(C.Structure):
    """ndt_feature_planes: where the planes of a feature pass go (host or device pointers; None: not wanted)"""
    _fields_ = [("id", C.c_void_p), ("position", C.c_void_p), ("normal", C.c_void_p), ("ray_o", C.c_void_p), ("ray_v", C.c_void_p)]


def feature_mask(features):
    """The NDT_FEATURE_* mask of an iterable of "id" / "position" / "normal" (or of a mask); ValueError for anything else or none."""
    if isinstance(features, int):
        mask = features
    else:
        mask = 0
        for name in features:
            if str(name) not in FEATURES:
                raise ValueError("feature %r is none of 'id', 'position', 'normal'" % (name,))
            mask |= FEATURES[str(name)]
    if mask <= 0 or mask & ~7:
        raise ValueError("feature mask %r: at least one of id 1, position 2, normal 4" % (mask,))
    return mask


def exr_features_bound(width, rows, dims, features=("id", "position", "normal"), pixel="half", depth_map=False):
    """ndt_hip_exr_features_bound: exr_bound for a file that also carries the feature channels of a dims-dimensional scene."""
    ep = exr_params(pixel)
    n = int(load_library().ndt_hip_exr_features_bound(int(width), int(rows), C.byref(ep), 1 if depth_map else 0, int(dims),
                                                      feature_mask(features)))
    if n < 0:
        raise ValueError("no EXR of %d x %d with the features of %d dimensions: a bad size, or samples beyond 2^31 - 1 bytes"
                         % (width, rows, dims))
    return n


class DenoiseParams(C.Structure):
    """ndt_denoise_params: iterations 1 .. 6, normal_power_log2 0 .. 8, the two sigmas finite and above 0"""
    _fields_ = [("iterations", C.c_int32), ("normal_power_log2", C.c_int32), ("sigma_colour", C.c_double), ("sigma_plane", C.c_double)]


def denoise_params(iterations=4, sigma_colour=0.25, sigma_plane=0.25, normal_power_log2=5):
    """The ndt_denoise_params of these values (the defaults are the library's); the library checks their ranges."""
    return DenoiseParams(int(iterations), int(normal_power_log2), float(sigma_colour), float(sigma_plane))


class VDenoiseParams(C.Structure):
    """ndt_vdenoise_params: iterations 1 .. 6, normal_power_log2 0 .. 8, k_colour and sigma_plane finite and above 0"""
    _fields_ = [("iterations", C.c_int32), ("normal_power_log2", C.c_int32), ("k_colour", C.c_double), ("sigma_plane", C.c_double)]


def vdenoise_params(iterations=4, k_colour=4.0, sigma_plane=0.25, normal_power_log2=5):
    """The ndt_vdenoise_params of these values (the defaults are the library's); the library checks their ranges."""
    return VDenoiseParams(int(iterations), int(normal_power_log2), float(k_colour), float(sigma_plane))


class AoParams(C.Structure):
    """ndt_ao_params: samples 1 .. 256, radius finite and >= 0 (0: no limit), any seed, strength 0 .. 1"""
    _fields_ = [("samples", C.c_int32), ("reserved", C.c_int32), ("radius", C.c_double), ("seed", C.c_uint64), ("strength", C.c_double)]


def ao_params(samples=16, radius=0.0, seed=0, strength=1.0):
    """The ndt_ao_params of these values (the defaults are the library's); the library checks their ranges."""
    return AoParams(int(samples), 0, float(radius), int(seed) & 0xffffffffffffffff, float(strength))


def exr_ao_bound(width, rows, dims, features=None, pixel="half", depth_map=False):
    """ndt_hip_exr_ao_bound: exr_features_bound for a file that also carries the channel AO; features may be None (no feature channel)."""
    ep = exr_params(pixel)
    n = int(load_library().ndt_hip_exr_ao_bound(int(width), int(rows), C.byref(ep), 1 if depth_map else 0, int(dims),
                                                feature_mask(features) if features else 0))
    if n < 0:
        raise ValueError("no EXR of %d x %d with AO and the features of %d dimensions: a bad size, or samples beyond 2^31 - 1 bytes"
                         % (width, rows, dims))
    return n


JPEG_SAMPLING = {"420": 0, "444": 1}


def jpeg_params(quality=95, sampling="420"):
    """The ndt_jpeg_params of a quality 1 .. 100 and a sampling "420" or "444"; ValueError for anything else."""
    if int(quality) != quality or not 1 <= quality <= 100:
        raise ValueError("JPEG quality %r is outside 1 .. 100" % (quality,))
    if str(sampling) not in JPEG_SAMPLING:
        raise ValueError("JPEG sampling %r is neither '420' nor '444'" % (sampling,))
    return JpegParams(int(quality), JPEG_SAMPLING[str(sampling)])


def jpeg_bound(width, rows, quality=95, sampling="420"):
    """ndt_hip_jpeg_bound: the largest file the device encoder can produce for a width x rows image (host arithmetic)."""
    jp = jpeg_params(quality, sampling)
    n = int(load_library().ndt_hip_jpeg_bound(int(width), int(rows), C.byref(jp)))
    if n < 0:
        raise ValueError("no JPEG of %d x %d: a side is empty or above 65535" % (width, rows))
    return n


def png_bound(width, rows):
    """ndt_hip_png_bound: the largest file the device encoder can produce for a width x rows image (host arithmetic)."""
    n = int(load_library().ndt_hip_png_bound(int(width), int(rows)))
    if n < 0:
        raise ValueError("no PNG of %d x %d: the size is empty or its filtered stream exceeds 2^31 - 1 bytes" % (width, rows))
    return n


def apng_bound(width, rows):
    """ndt_hip_apng_bound: the most bytes one frame can append to the animated PNG of a width x rows canvas (host arithmetic)."""
    n = int(load_library().ndt_hip_apng_bound(int(width), int(rows)))
    if n < 0:
        raise ValueError("no animated PNG of %d x %d: the size is empty or its filtered stream exceeds 2^31 - 1 bytes" % (width, rows))
    return n


def png16_bound(width, rows, channels=4):
    """ndt_hip_png16_bound: the largest 16-bit file the device encoder can produce for a width x rows image of 4 (RGBA) or 1 (grey)
    channels (host arithmetic)."""
    n = int(load_library().ndt_hip_png16_bound(int(width), int(rows), int(channels)))
    if n < 0:
        raise ValueError("no 16-bit PNG of %d x %d x %d: the channels are neither 1 nor 4, the size is empty or its filtered stream "
                         "exceeds 2^31 - 1 bytes" % (width, rows, channels))
    return n


def pack_boxes(dims, lower, upper, finite):
    """The flat arrays ndt_hip_build_kdtree / ndt_host_build_kdtree take: (n, lower [n, dims], upper [n, dims], finite uint8 [n])."""
    lower = np.ascontiguousarray(lower, dtype=np.float64).reshape(-1, int(dims))
    upper = np.ascontiguousarray(upper, dtype=np.float64).reshape(-1, int(dims))
    finite = np.ascontiguousarray(np.asarray(finite) != 0, dtype=np.uint8).reshape(-1)
    if not lower.shape == upper.shape == (finite.shape[0], int(dims)):
        raise ValueError("lower and upper must be [n, %d] and finite [n]" % dims)
    return finite.shape[0], lower, upper, finite


def pack_point_lists(dims, lists):
    """The flat arrays ndt_hip_fit_spheres / ndt_host_fit_spheres take, from a sequence of (points [k, dims], radii [k]) pairs
    in the order bounds_list_optimal walks each list: (first int64 [n + 1], points float64 [total, dims], radii float64 [total])."""
    first = np.zeros(len(lists) + 1, dtype=np.int64)
    for i, (pts, rad) in enumerate(lists):
        pts = np.asarray(pts, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] != dims or np.asarray(rad).shape != (pts.shape[0],):
            raise ValueError("list %d: points must be [k, %d] and radii [k]" % (i, dims))
        first[i + 1] = first[i] + pts.shape[0]
    points = np.zeros((int(first[-1]), dims), dtype=np.float64)
    radii = np.zeros(int(first[-1]), dtype=np.float64)
    for i, (pts, rad) in enumerate(lists):
        points[first[i]:first[i + 1]] = pts
        radii[first[i]:first[i + 1]] = rad
    return first, points, radii


def hcube_hull_box(fs, obj):
    """The hull box libndt_hip derives for hcube `obj` of FlatScene `fs` (host only, no GPU):
    (axes[N,N], centre[N], half[N]) or None when the hcube gets no box."""
    import numpy as np
    lib = load_library()
    n = fs.dims
    rows = np.zeros((n, n + 2), dtype=np.float64)
    rc = lib.ndt_hip_hcube_hull_box(fs.byref(), int(obj), rows.ctypes.data)
    if rc < 0:
        raise NdtHipError(rc, (lib.ndt_hip_last_error() or b"").decode())
    if rc == 0:
        return None
    return rows[:, :n].copy(), rows[:, n].copy(), rows[:, n + 1].copy()


def item_boxes(fs):
    """ndt_hip_item_boxes: (frame [d, d], rows [n_items, d, 2], has [n_items] bool) or None when the scene has no boxed item."""
    lib = load_library()
    d, n = fs.dims, fs.struct.n_items
    frame = np.zeros((d, d))
    rows = np.zeros((max(n, 1), d, 2))
    has = np.zeros(max(n, 1), dtype=np.uint8)
    rc = lib.ndt_hip_item_boxes(fs.byref(), frame.ctypes.data, rows.ctypes.data, has.ctypes.data)
    if rc < 0:
        raise NdtHipError(rc, (lib.ndt_hip_last_error() or b"").decode())
    if rc == 0:
        return None
    return frame, rows[:n], has[:n].astype(bool)


def check_scene(fs):
    """ndt_hip_check_scene: what ndt_hip_upload_scene accepts (host only, no GPU, no context).  Returns None for a scene upload
    would take and raises NdtHipError with upload's code and message for one it would refuse."""
    lib = load_library()
    rc = lib.ndt_hip_check_scene(fs.byref())
    if rc != 0:
        raise NdtHipError(rc, (lib.ndt_hip_last_error() or b"").decode())


def hcube_face_boxes(fs, obj):
    """The boxes of the single faces of hcube `obj` in its hull box's frame (host only, no GPU), for an hcube of any number of
    faces: (centre[F,N], half[F,N], possible[F] bool) or None when the hcube gets no face boxes."""
    import numpy as np
    lib = load_library()
    n = fs.dims
    count = lib.ndt_hip_hcube_face_boxes_all(fs.byref(), int(obj), 0, None, None)
    if count < 0:
        raise NdtHipError(int(count), (lib.ndt_hip_last_error() or b"").decode())
    if count == 0:
        return None
    rows = np.zeros((count, n, 2), dtype=np.float64)
    possible = np.zeros(count, dtype=np.uint8)
    rc = lib.ndt_hip_hcube_face_boxes_all(fs.byref(), int(obj), count, rows.ctypes.data, possible.ctypes.data)
    assert rc == count
    return rows[:, :, 0].copy(), rows[:, :, 1].copy(), possible.astype(bool)


def hcube_face_tree(fs, obj):
    """The hierarchy over the face boxes of hcube `obj` (host only, no GPU): a list, level j = 1 .. top, of
    (centre[K_j, N], half[K_j, N]) for the aligned runs of 2^j faces; None when the hcube gets no face boxes."""
    import numpy as np
    lib = load_library()
    n = fs.dims
    top = C.c_int32(0)
    off = (C.c_int32 * 32)()
    count = lib.ndt_hip_hcube_face_tree(fs.byref(), int(obj), 0, None, off, C.byref(top))
    if count < 0:
        raise NdtHipError(int(count), (lib.ndt_hip_last_error() or b"").decode())
    if count == 0:
        return None
    rows = np.zeros((count, n, 2), dtype=np.float64)
    rc = lib.ndt_hip_hcube_face_tree(fs.byref(), int(obj), count, rows.ctypes.data, off, C.byref(top))
    assert rc == count
    levels = []
    for j in range(1, top.value + 1):
        end = off[j + 1] if j < top.value else count
        levels.append((rows[off[j]:end, :, 0].copy(), rows[off[j]:end, :, 1].copy()))
    return levels


def hcube_face_groups(fs, obj):
    """The index of hcube `obj`'s faces by the hull axes their boxes are thin on (host only, no GPU):
    (clusters[N, 2, 2] = per axis and side {centre, half}, table[2^N, 2] = {start, count} per subset of the axes into members,
    face_set[n_faces], members); None when the hcube gets no face boxes."""
    import numpy as np
    lib = load_library()
    n = fs.dims
    nf = fs.objects[int(obj)]["n_obj"]
    clusters = np.zeros((n, 2, 2), dtype=np.float64)
    table = np.zeros((1 << n, 2), dtype=np.int32)
    face_set = np.zeros(max(nf, 1), dtype=np.int32)
    members = np.zeros(max(nf, 1), dtype=np.int32)
    rc = lib.ndt_hip_hcube_face_groups(fs.byref(), int(obj), clusters.ctypes.data, table.ctypes.data, face_set.ctypes.data, members.ctypes.data)
    if rc < 0:
        raise NdtHipError(int(rc), (lib.ndt_hip_last_error() or b"").decode())
    if rc == 0:
        return None
    return clusters, table, face_set[:rc], members[:int((face_set[:rc] >= 0).sum())]


class NdtHip:
    """One rendering context = one MI355X + one HIP stream (ndt_hip_create)."""

    def __init__(self, device=0):
        self.lib = load_library()
        self.ctx = C.c_void_p()
        self._check(self.lib.ndt_hip_create(int(device), C.byref(self.ctx)))
        self.device = int(device)
        self.scene = None

    def _check(self, rc):
        if rc != 0:
            raise NdtHipError(rc, (self.lib.ndt_hip_last_error() or b"").decode())

    def close(self):
        if self.ctx:
            self.lib.ndt_hip_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self):
        return self.lib.ndt_hip_stream(self.ctx)

    def synchronize(self):
        self._check(self.lib.ndt_hip_synchronize(self.ctx))

    def set_option(self, name, value):
        """ndt_hip_set_option: "pipeline" (0 auto, 1 levels, 2 stream), "hull_box", "face_box", "debug_levels", ..."""
        self._check(self.lib.ndt_hip_set_option(self.ctx, name.encode(), int(value)))

    def multi_path_taken(self):
        """ndt_hip_multi_path_taken: how this context's rows reached the frame in the last render_multi (MULTI_*)."""
        return int(self.lib.ndt_hip_multi_path_taken(self.ctx))

    def upload_scene(self, fs):
        self.scene = None        # (a refused upload leaves the context without a scene: include/ndt_hip.h "What upload accepts")
        self._check(self.lib.ndt_hip_upload_scene(self.ctx, fs.byref()))
        self.scene = fs          # keep the arrays alive; also gives dims

    def _dims(self):
        """Dimensions of the uploaded scene; without one, the error the library itself gives a call out of order."""
        if self.scene is None:
            raise NdtHipError(NDT_E_STATE, "no scene uploaded")
        return self.scene.dims

    def params(self, width, height, depth, row_begin=0, row_step=1, specular=1, profile=0, aa=None, stereo=0, samples=1):
        p = RenderParams(width, height, depth, int(samples), row_begin, row_step, specular, profile)
        p.stereo = int(stereo)      # ndt_stereo_mode: 0 mono, 1 side by side, 2 over/under, 3 anaglyph, 4 frame packing (2205 lines)
        if aa is not None:
            # Whitted's recursive anti-aliasing, `-a diff,depth` (ndt.c:655-733)
            p.recursive_aa, p.aa_diff, p.aa_depth = 1, int(aa[0]), int(aa[1])
        return p

    def render(self, width, height, depth, row_begin=0, row_step=1, specular=1, profile=0, aa=None, stereo=0,
               depth_map=False, samples=1, ssaa=None):
        """render_image for a row shard; returns ((rows, width, 4) float64 host array, RenderStats).
        aa = (aa_diff, aa_depth) switches recursive anti-aliasing on; stereo = ndt_stereo_mode;
        depth_map=True returns (rgba, (rows, width) depth map, stats); ssaa = K supersamples K x K on the device (render_ssaa:
        the library refuses it beside aa)."""
        if ssaa is not None:
            p = self.params(width, height, depth, row_begin, row_step, specular, profile, aa, stereo, samples)
            rows = shard_rows(height, row_begin, row_step)
            out = np.zeros((rows, width, 4), dtype=np.float64)
            dm = np.zeros((rows, width), dtype=np.float64) if depth_map else None
            st = RenderStats()
            self._check(self.lib.ndt_hip_render_ssaa(self.ctx, C.byref(p), int(ssaa), out.ctypes.data, dm.ctypes.data if depth_map else None,
                                                     C.byref(st)))
            return (out, dm, st) if depth_map else (out, st)
        p = self.params(width, height, depth, row_begin, row_step, specular, profile, aa, stereo, samples)
        if depth_map:
            rows = shard_rows(height, row_begin, row_step)
            out = np.zeros((rows, width, 4), dtype=np.float64)
            dm = np.zeros((rows, width), dtype=np.float64)
            st = RenderStats()
            self._check(self.lib.ndt_hip_render_depth(self.ctx, C.byref(p), out.ctypes.data_as(C.c_void_p),
                                                      dm.ctypes.data_as(C.c_void_p), C.byref(st)))
            return out, dm, st
        rows = shard_rows(height, row_begin, row_step)
        out = np.zeros((rows, width, 4), dtype=np.float64)
        st = RenderStats()
        self._check(self.lib.ndt_hip_render(self.ctx, C.byref(p), out.ctypes.data_as(C.c_void_p), C.byref(st)))
        return out, st

    def render_device(self, d_rgba_ptr, width, height, depth, row_begin=0, row_step=1, specular=1, profile=0, aa=None, stereo=0,
                      samples=1):
        """Same, output left in HBM at raw device pointer `d_rgba_ptr` (rows*width*4 doubles)."""
        p = self.params(width, height, depth, row_begin, row_step, specular, profile, aa, stereo, samples)
        st = RenderStats()
        self._check(self.lib.ndt_hip_render_device(self.ctx, C.byref(p), C.c_void_p(d_rgba_ptr), C.byref(st)))
        return st

    def render_rgba8(self, width, height, depth, **kw):
        """render_image + the reference's save-time quantisation on the device: (rows, width, 4) uint8 host array, stats."""
        p = self.params(width, height, depth, **kw)
        rows = shard_rows(height, p.row_begin, p.row_step)
        out = np.zeros((rows, width, 4), dtype=np.uint8)
        st = RenderStats()
        self._check(self.lib.ndt_hip_render_rgba8(self.ctx, C.byref(p), out.ctypes.data_as(C.c_void_p), C.byref(st)))
        return out, st

    def render_rgba8_async(self, host_ptr, width, height, depth, **kw):
        """ndt_hip_render_rgba8_async: the frame's bytes travel to pinned host memory at `host_ptr` behind the next call's
        rendering; read them after render_rgba8_wait()."""
        p = self.params(width, height, depth, **kw)
        st = RenderStats()
        self._check(self.lib.ndt_hip_render_rgba8_async(self.ctx, C.byref(p), C.c_void_p(host_ptr), C.byref(st)))
        return st

    def render_rgba8_wait(self):
        self._check(self.lib.ndt_hip_render_rgba8_wait(self.ctx))

    def encode_png(self, rgba8, cap=None):
        """ndt_hip_encode_png: the complete PNG file of a (rows, width, 4) uint8 host image, compressed on this context's GPU.
        Returns the file's bytes; self.png_stats keeps the ndt_png_stats.  cap: room offered (default: ndt_hip_png_bound)."""
        rgba8 = np.ascontiguousarray(rgba8, dtype=np.uint8)
        if rgba8.ndim != 3 or rgba8.shape[2] != 4:
            raise ValueError("rgba8 must be (rows, width, 4)")
        rows, width = rgba8.shape[:2]
        cap = png_bound(width, rows) if cap is None else int(cap)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        self.png_stats = PngStats()
        self._check(self.lib.ndt_hip_encode_png(self.ctx, rgba8.ctypes.data, width, rows, out.ctypes.data, cap, C.byref(self.png_stats)))
        return out[:self.png_stats.png_bytes].tobytes()

    def encode_png_device(self, d_rgba8_ptr, width, rows, cap=None):
        """ndt_hip_encode_png_device: the same for width * rows * 4 bytes at raw device pointer `d_rgba8_ptr`."""
        cap = png_bound(width, rows) if cap is None else int(cap)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        self.png_stats = PngStats()
        self._check(self.lib.ndt_hip_encode_png_device(self.ctx, C.c_void_p(d_rgba8_ptr), int(width), int(rows), out.ctypes.data, cap,
                                                       C.byref(self.png_stats)))
        return out[:self.png_stats.png_bytes].tobytes()

    def render_png(self, width, height, depth, **kw):
        """ndt_hip_render_png: render_rgba8 with the device's PNG encoder in place of the download.  Returns (the file's bytes,
        RenderStats); self.png_stats keeps the ndt_png_stats.  The PNG's height is the row shard's."""
        p = self.params(width, height, depth, **kw)
        rows = shard_rows(height, p.row_begin, p.row_step)
        cap = png_bound(width, rows)
        out = np.zeros(cap, dtype=np.uint8)
        st = RenderStats()
        self.png_stats = PngStats()
        self._check(self.lib.ndt_hip_render_png(self.ctx, C.byref(p), out.ctypes.data, cap, C.byref(self.png_stats), C.byref(st)))
        return out[:self.png_stats.png_bytes].tobytes(), st

    def encode_png16(self, samples, cap=None):
        """ndt_hip_encode_png16: the complete 16-bit PNG file of a (rows, width, 4) RGBA or (rows, width) grey host image of uint16
        values, compressed on this context's GPU.  Returns the file's bytes; self.png_stats keeps the ndt_png_stats."""
        samples = np.asarray(samples)
        if samples.dtype != np.uint16 or not (samples.ndim == 2 or (samples.ndim == 3 and samples.shape[2] == 4)):
            raise ValueError("samples must be uint16, (rows, width, 4) or (rows, width)")
        rows, width = samples.shape[:2]
        channels = 4 if samples.ndim == 3 else 1
        wire = np.ascontiguousarray(samples.astype(">u2"))          # file byte order
        cap = png16_bound(width, rows, channels) if cap is None else int(cap)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        self.png_stats = PngStats()
        self._check(self.lib.ndt_hip_encode_png16(self.ctx, wire.ctypes.data, width, rows, channels, out.ctypes.data, cap,
                                                  C.byref(self.png_stats)))
        return out[:self.png_stats.png_bytes].tobytes()

    def encode_png16_device(self, d_samples_ptr, width, rows, channels, cap=None):
        """ndt_hip_encode_png16_device: the same for width * rows * channels samples in file byte order at raw device pointer
        `d_samples_ptr`."""
        cap = png16_bound(width, rows, channels) if cap is None else int(cap)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        self.png_stats = PngStats()
        self._check(self.lib.ndt_hip_encode_png16_device(self.ctx, C.c_void_p(d_samples_ptr), int(width), int(rows), int(channels),
                                                         out.ctypes.data, cap, C.byref(self.png_stats)))
        return out[:self.png_stats.png_bytes].tobytes()

    def quantize16_device(self, d_rgba_ptr, d_rgba16_ptr, n_pixels):
        """ndt_hip_quantize16_device: n_pixels * 4 doubles at `d_rgba_ptr` to n_pixels * 8 bytes of 16-bit samples in file byte
        order at `d_rgba16_ptr` (on the context's stream: synchronize() before reading them)."""
        self._check(self.lib.ndt_hip_quantize16_device(self.ctx, C.c_void_p(d_rgba_ptr), C.c_void_p(d_rgba16_ptr), int(n_pixels)))

    def depth_grey16_device(self, d_depth_ptr, n_pixels, d_grey16_ptr):
        """ndt_hip_depth_grey16_device: depth_rgba8_device with one 16-bit grey sample a pixel, in file byte order.  Returns (lo, hi)."""
        rng = np.zeros(2, dtype=np.float64)
        self._check(self.lib.ndt_hip_depth_grey16_device(self.ctx, C.c_void_p(d_depth_ptr), int(n_pixels), C.c_void_p(d_grey16_ptr),
                                                         rng.ctypes.data))
        return rng

    def render_png16(self, width, height, depth, **kw):
        """ndt_hip_render_png16: render_png at 16 bits a sample.  Returns (the file's bytes, RenderStats); self.png_stats keeps the
        ndt_png_stats."""
        p = self.params(width, height, depth, **kw)
        rows = shard_rows(height, p.row_begin, p.row_step)
        cap = png16_bound(width, rows, 4)
        out = np.zeros(cap, dtype=np.uint8)
        st = RenderStats()
        self.png_stats = PngStats()
        self._check(self.lib.ndt_hip_render_png16(self.ctx, C.byref(p), out.ctypes.data, cap, C.byref(self.png_stats), C.byref(st)))
        return out[:self.png_stats.png_bytes].tobytes(), st

    def render_png16_depth(self, width, height, depth, cap=None, depth_cap=None, **kw):
        """ndt_hip_render_png16_depth: the image as a 16-bit RGBA file and the map as a 16-bit grey one.  Returns (file, file,
        [lo, hi], RenderStats); self.png_stats keeps the two ndt_png_stats (image, map)."""
        p = self.params(width, height, depth, **kw)
        rows = shard_rows(height, p.row_begin, p.row_step)
        cap = png16_bound(width, rows, 4) if cap is None else int(cap)
        depth_cap = png16_bound(width, rows, 1) if depth_cap is None else int(depth_cap)
        out, dpng = np.zeros(max(cap, 1), dtype=np.uint8), np.zeros(max(depth_cap, 1), dtype=np.uint8)
        rng = np.zeros(2, dtype=np.float64)
        st = RenderStats()
        self.png_stats = (PngStats * 2)()
        self._check(self.lib.ndt_hip_render_png16_depth(self.ctx, C.byref(p), out.ctypes.data, cap, dpng.ctypes.data, depth_cap,
                                                        C.byref(self.png_stats), rng.ctypes.data, C.byref(st)))
        return out[:self.png_stats[0].png_bytes].tobytes(), dpng[:self.png_stats[1].png_bytes].tobytes(), rng, st

    def render_ssaa_png16(self, width, height, depth, ssaa, depth_map=False, **kw):
        """ndt_hip_render_ssaa_png16 (depth_map=True: ndt_hip_render_ssaa_png16_depth): the supersampled frame as a 16-bit file:
        (the file's bytes, stats), or (file, the map's file, [lo, hi], stats); self.png_stats keeps the record(s)."""
        p, rows = self._ssaa_params(width, height, depth, kw)
        cap = png16_bound(width, rows, 4)
        out = np.zeros(cap, dtype=np.uint8)
        st = RenderStats()
        if not depth_map:
            self.png_stats = PngStats()
            self._check(self.lib.ndt_hip_render_ssaa_png16(self.ctx, C.byref(p), int(ssaa), out.ctypes.data, cap, C.byref(self.png_stats),
                                                           C.byref(st)))
            return out[:self.png_stats.png_bytes].tobytes(), st
        depth_cap = png16_bound(width, rows, 1)
        dpng = np.zeros(depth_cap, dtype=np.uint8)
        rng = np.zeros(2, dtype=np.float64)
        self.png_stats = (PngStats * 2)()
        self._check(self.lib.ndt_hip_render_ssaa_png16_depth(self.ctx, C.byref(p), int(ssaa), out.ctypes.data, cap, dpng.ctypes.data,
                                                             depth_cap, C.byref(self.png_stats), rng.ctypes.data, C.byref(st)))
        return out[:self.png_stats[0].png_bytes].tobytes(), dpng[:self.png_stats[1].png_bytes].tobytes(), rng, st

    def encode_exr(self, rgba, depth=None, pixel="half", cap=None):
        """ndt_hip_encode_exr: the complete OpenEXR file of a (rows, width, 4) float64 host image in linear light and, with `depth`,
        a (rows, width) float64 map as its Z channel, made on this context's GPU.  Returns the file's bytes; self.exr_stats keeps
        the ndt_exr_stats.  cap: room offered (default: ndt_hip_exr_bound)."""
        rgba = np.ascontiguousarray(rgba, dtype=np.float64)
        if rgba.ndim != 3 or rgba.shape[2] != 4:
            raise ValueError("rgba must be (rows, width, 4)")
        rows, width = rgba.shape[:2]
        if depth is not None:
            depth = np.ascontiguousarray(depth, dtype=np.float64)
            if depth.shape != (rows, width):
                raise ValueError("depth must be (rows, width)")
        ep = exr_params(pixel)
        cap = exr_bound(width, rows, pixel, depth is not None) if cap is None else int(cap)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        self.exr_stats = ExrStats()
        self._check(self.lib.ndt_hip_encode_exr(self.ctx, rgba.ctypes.data, depth.ctypes.data if depth is not None else None, width, rows,
                                                C.byref(ep), out.ctypes.data, cap, C.byref(self.exr_stats)))
        return out[:self.exr_stats.file_bytes].tobytes()

    def encode_exr_device(self, d_rgba_ptr, d_depth_ptr, width, rows, pixel="half", cap=None):
        """ndt_hip_encode_exr_device: the same for rows * width * 4 doubles at raw device pointer `d_rgba_ptr` and, unless
        `d_depth_ptr` is None, rows * width doubles of map there."""
        ep = exr_params(pixel)
        cap = exr_bound(width, rows, pixel, d_depth_ptr is not None) if cap is None else int(cap)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        self.exr_stats = ExrStats()
        self._check(self.lib.ndt_hip_encode_exr_device(self.ctx, C.c_void_p(d_rgba_ptr), C.c_void_p(d_depth_ptr) if d_depth_ptr else None,
                                                       int(width), int(rows), C.byref(ep), out.ctypes.data, cap, C.byref(self.exr_stats)))
        return out[:self.exr_stats.file_bytes].tobytes()

    def render_exr(self, width, height, depth, pixel="half", depth_map=False, features=None, cap=None, ao=None, **kw):
        """ndt_hip_render_exr: render() with the device's OpenEXR encoder in place of the download; depth_map=True adds the map as
        the file's Z channel.  features (names of FEATURES, e.g. ("id", "position", "normal")): ndt_hip_render_exr_features, the
        primary hit of every pixel as the channels id, P.*, N.* of the file.  Returns (the file's bytes, RenderStats);
        self.exr_stats keeps the ndt_exr_stats.  The file's height is the row shard's.  cap: room offered (default: the bound).
        ao (a dict of ao_params' arguments, or True for the defaults): ndt_hip_render_exr_ao, the file with the channel AO, its colour
        multiplied by the plane at the dict's strength; features may then be None."""
        p = self.params(width, height, depth, **kw)
        rows = shard_rows(height, p.row_begin, p.row_step)
        ep = exr_params(pixel)
        if ao is not None and ao is not False:
            ap = ao_params(**({} if ao is True else dict(ao)))
            cap = exr_ao_bound(width, rows, self._dims(), features, pixel, depth_map) if cap is None else int(cap)
            out = np.zeros(max(cap, 1), dtype=np.uint8)
            st = RenderStats()
            self.exr_stats = ExrStats()
            self._check(self.lib.ndt_hip_render_exr_ao(self.ctx, C.byref(p), C.byref(ep), 1 if depth_map else 0,
                                                       feature_mask(features) if features else 0, C.byref(ap), out.ctypes.data, cap,
                                                       C.byref(self.exr_stats), C.byref(st)))
            return out[:self.exr_stats.file_bytes].tobytes(), st
        if cap is None:
            cap = exr_features_bound(width, rows, self._dims(), features, pixel, depth_map) if features else exr_bound(width, rows, pixel, depth_map)
        out = np.zeros(int(cap), dtype=np.uint8)
        st = RenderStats()
        self.exr_stats = ExrStats()
        if features:
            self._check(self.lib.ndt_hip_render_exr_features(self.ctx, C.byref(p), C.byref(ep), 1 if depth_map else 0, feature_mask(features),
                                                             out.ctypes.data, int(cap), C.byref(self.exr_stats), C.byref(st)))
        else:
            self._check(self.lib.ndt_hip_render_exr(self.ctx, C.byref(p), C.byref(ep), 1 if depth_map else 0, out.ctypes.data, int(cap),
                                                    C.byref(self.exr_stats), C.byref(st)))
        return out[:self.exr_stats.file_bytes].tobytes(), st

    def render_ssaa_exr(self, width, height, depth, ssaa, pixel="half", depth_map=False, features=None, **kw):
        """ndt_hip_render_ssaa_exr: the supersampled frame as an OpenEXR file (Z: sub-sample (0, 0)'s map): (the file's bytes, stats);
        self.exr_stats keeps the record.  features: ndt_hip_render_ssaa_exr_features, the plain frame's feature channels beside it."""
        p, rows = self._ssaa_params(width, height, depth, kw)
        ep = exr_params(pixel)
        cap = exr_features_bound(width, rows, self._dims(), features, pixel, depth_map) if features else exr_bound(width, rows, pixel, depth_map)
        out = np.zeros(cap, dtype=np.uint8)
        st = RenderStats()
        self.exr_stats = ExrStats()
        if features:
            self._check(self.lib.ndt_hip_render_ssaa_exr_features(self.ctx, C.byref(p), int(ssaa), C.byref(ep), 1 if depth_map else 0,
                                                                  feature_mask(features), out.ctypes.data, cap, C.byref(self.exr_stats),
                                                                  C.byref(st)))
        else:
            self._check(self.lib.ndt_hip_render_ssaa_exr(self.ctx, C.byref(p), int(ssaa), C.byref(ep), 1 if depth_map else 0, out.ctypes.data,
                                                         cap, C.byref(self.exr_stats), C.byref(st)))
        return out[:self.exr_stats.file_bytes].tobytes(), st

    def render_features(self, width, height, depth, rays=False, **kw):
        """ndt_hip_render_features: what every pixel of the frame shows -- the closest hit of its primary ray.  Returns a dict of
        arrays: "id" (rows, width) int32, object index + 1 and 0 for no hit; "position" and "normal" (dims, rows, width) float64,
        zero where id is 0; with rays=True also "ray_o" and "ray_v" (dims, rows, width), the rays themselves.  kw: as render()'s
        (row shards, stereo 1 / 2); frames without one primary ray a pixel (aa, samples > 1, anaglyph) are refused."""
        p = self.params(width, height, depth, **kw)
        rows = shard_rows(height, p.row_begin, p.row_step)
        d = self._dims()
        out = {"id": np.zeros((rows, width), dtype=np.int32), "position": np.zeros((d, rows, width)), "normal": np.zeros((d, rows, width))}
        if rays:
            out["ray_o"], out["ray_v"] = np.zeros((d, rows, width)), np.zeros((d, rows, width))
        planes = FeaturePlanes(*[out[k].ctypes.data if k in out else None for k in ("id", "position", "normal", "ray_o", "ray_v")])
        st = RenderStats()
        self._check(self.lib.ndt_hip_render_features(self.ctx, C.byref(p), C.byref(planes), C.byref(st)))
        return out

    def features_launches(self):
        """ndt_hip_features_launches: kernel launches of the context's last feature pass."""
        return int(self.lib.ndt_hip_features_launches(self.ctx))

    def encode_exr_features_device(self, d_rgba_ptr, d_depth_ptr, d_planes, dims, features, width, rows, pixel="half", cap=None):
        """ndt_hip_encode_exr_features_device: the file of device doubles at `d_rgba_ptr` (and the map at `d_depth_ptr`, or None)
        with the feature channels of `features` taken from the device planes `d_planes` names: a dict "id" / "position" / "normal"
        of raw device pointers.  Returns the file's bytes; self.exr_stats keeps the record."""
        ep = exr_params(pixel)
        mask = feature_mask(features)
        cap = exr_features_bound(width, rows, dims, mask, pixel, d_depth_ptr is not None) if cap is None else int(cap)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        planes = FeaturePlanes(d_planes.get("id"), d_planes.get("position"), d_planes.get("normal"), None, None)
        self.exr_stats = ExrStats()
        self._check(self.lib.ndt_hip_encode_exr_features_device(self.ctx, C.c_void_p(d_rgba_ptr), C.c_void_p(d_depth_ptr) if d_depth_ptr else None,
                                                                C.byref(planes), int(dims), mask, int(width), int(rows), C.byref(ep),
                                                                out.ctypes.data, cap, C.byref(self.exr_stats)))
        return out[:self.exr_stats.file_bytes].tobytes()

    def denoise(self, d_rgba_in_ptr, d_planes, dims, width, rows, d_rgba_out_ptr=None, **dn):
        """ndt_hip_denoise_device: the edge-avoiding a-trous filter alone, on rows x width x 4 device doubles at `d_rgba_in_ptr`,
        guided by the device planes `d_planes` names (a dict "id" / "position" / "normal" of raw device pointers), into
        `d_rgba_out_ptr` (default: in place).  dn: iterations, sigma_colour, sigma_plane, normal_power_log2."""
        dp = denoise_params(**dn)
        planes = FeaturePlanes(d_planes.get("id"), d_planes.get("position"), d_planes.get("normal"), None, None)
        out = d_rgba_in_ptr if d_rgba_out_ptr is None else d_rgba_out_ptr
        self._check(self.lib.ndt_hip_denoise_device(self.ctx, C.c_void_p(d_rgba_in_ptr), C.byref(planes), int(dims), int(width), int(rows),
                                                    C.byref(dp), C.c_void_p(out)))

    def denoise_launches(self):
        """ndt_hip_denoise_launches: kernel launches of the context's last denoised frame (the feature pass's and the iterations')."""
        return int(self.lib.ndt_hip_denoise_launches(self.ctx))

    def denoise_ms(self):
        """ndt_hip_denoise_ms: summed device time of its iterations."""
        return float(self.lib.ndt_hip_denoise_ms(self.ctx))

    def render_denoised(self, width, height, depth, sink=None, iterations=4, sigma_colour=0.25, sigma_plane=0.25, normal_power_log2=5,
                        d_rgba_ptr=None, quality=95, sampling="420", pixel="half", cap=None, **kw):
        """ndt_hip_render_denoised*: the frame render(**kw) gives (samples and all), denoised on the device by the a-trous filter,
        guided by the feature pass of the same frame with samples = 1.  sink None: ((rows, width, 4) float64, RenderStats);
        "device": left at raw device pointer `d_rgba_ptr`, returns the stats; "rgba8": the (rows, width, 4) uint8 image;
        "png" / "jpeg" / "exr": the file's bytes (self.png_stats / jpeg_stats / exr_stats keep the record) -- each with the stats."""
        p = self.params(width, height, depth, **kw)
        dp = denoise_params(iterations, sigma_colour, sigma_plane, normal_power_log2)
        return self._staged_sink("ndt_hip_render_denoised", (self.ctx, C.byref(p), C.byref(dp)), sink, (None, "device", "rgba8", "png", "jpeg", "exr"),
                                 shard_rows(height, p.row_begin, p.row_step), width, device=(d_rgba_ptr,), quality=quality, sampling=sampling,
                                 pixel=pixel, cap=cap)

    def render_moments(self, width, height, depth, **kw):
        """ndt_hip_render_moments: the frame render(**kw) gives, bit for bit, and what the adaptive loop consumed for it: returns
        ((rows, width, 4) float64, count (rows, width) int32 -- the samples of every pixel --, sum_sq (3, rows, width) float64 -- the
        sums of their squared r, g, b --, RenderStats).  Option "sample_cap" bounds the counts."""
        p = self.params(width, height, depth, **kw)
        rows = shard_rows(height, p.row_begin, p.row_step)
        out = np.zeros((rows, width, 4), dtype=np.float64)
        count = np.zeros((rows, width), dtype=np.int32)
        sum_sq = np.zeros((3, rows, width), dtype=np.float64)
        st = RenderStats()
        self._check(self.lib.ndt_hip_render_moments(self.ctx, C.byref(p), out.ctypes.data, count.ctypes.data, sum_sq.ctypes.data, C.byref(st)))
        return out, count, sum_sq, st

    def sample_variance(self, d_rgba_ptr, d_count_ptr, d_sum_sq_ptr, width, rows, d_variance_ptr):
        """ndt_hip_sample_variance_device: the variance of every pixel's mean, summed over r, g, b, from the moments at raw device
        pointers, into rows * width doubles at `d_variance_ptr`."""
        self._check(self.lib.ndt_hip_sample_variance_device(self.ctx, C.c_void_p(d_rgba_ptr), C.c_void_p(d_count_ptr), C.c_void_p(d_sum_sq_ptr),
                                                            int(width), int(rows), C.c_void_p(d_variance_ptr)))

    def vdenoise(self, d_rgba_in_ptr, d_planes, d_variance_ptr, dims, width, rows, d_rgba_out_ptr=None, d_variance_out_ptr=None, **vd):
        """ndt_hip_vdenoise_device: the variance-guided a-trous filter alone, on rows x width x 4 device doubles at `d_rgba_in_ptr` and
        the rows x width variance plane at `d_variance_ptr`, guided by the device planes `d_planes` names, into `d_rgba_out_ptr`
        (default: in place) and, unless None, the propagated plane into `d_variance_out_ptr`.  vd: iterations, k_colour, sigma_plane,
        normal_power_log2."""
        vp = vdenoise_params(**vd)
        planes = FeaturePlanes(d_planes.get("id"), d_planes.get("position"), d_planes.get("normal"), None, None)
        out = d_rgba_in_ptr if d_rgba_out_ptr is None else d_rgba_out_ptr
        self._check(self.lib.ndt_hip_vdenoise_device(self.ctx, C.c_void_p(d_rgba_in_ptr), C.byref(planes), C.c_void_p(d_variance_ptr), int(dims),
                                                     int(width), int(rows), C.byref(vp), C.c_void_p(out),
                                                     C.c_void_p(d_variance_out_ptr) if d_variance_out_ptr else None))

    def render_vdenoised(self, width, height, depth, sink=None, iterations=4, k_colour=4.0, sigma_plane=0.25, normal_power_log2=5,
                         d_rgba_ptr=None, quality=95, sampling="420", pixel="half", cap=None, **kw):
        """ndt_hip_render_vdenoised*: the frame render(**kw) gives, denoised on the device by the variance-guided a-trous filter: the
        width of its colour weight comes from the sample moments of the frame itself, pixel by pixel.  Sinks and answers as
        render_denoised's; denoise_launches() is 5 + iterations afterwards."""
        p = self.params(width, height, depth, **kw)
        vp = vdenoise_params(iterations, k_colour, sigma_plane, normal_power_log2)
        return self._staged_sink("ndt_hip_render_vdenoised", (self.ctx, C.byref(p), C.byref(vp)), sink, (None, "device", "rgba8", "png", "jpeg", "exr"),
                                 shard_rows(height, p.row_begin, p.row_step), width, device=(d_rgba_ptr,), quality=quality, sampling=sampling,
                                 pixel=pixel, cap=cap)

    def _staged_sink(self, stem, head, sink, sinks, rows, width, device=(), extra=(), quality=95, sampling="420", pixel="half", cap=None):
        """The sink ladder of the entries that stage a frame on the device -- <stem>, <stem>_device, _rgba8, _png, _jpeg, _exr, each
        called with `head` in front: allocates the output, keeps the file's record in self.png_stats / jpeg_stats / exr_stats, slices
        the file.  sinks: those `stem` has; device: the raw device pointers of "device"; extra: further host arrays of sink None,
        returned behind the image.  Every answer ends with the RenderStats."""
        if sink not in sinks:
            raise ValueError("sink %r is none of %s" % (sink, ", ".join(repr(name) for name in sinks)))
        st = RenderStats()
        if sink is None:
            out = np.zeros((rows, width, 4), dtype=np.float64)
            self._check(getattr(self.lib, stem)(*head, out.ctypes.data, *[a.ctypes.data for a in extra], C.byref(st)))
            return (out,) + tuple(extra) + (st,)
        if sink == "device":
            self._check(getattr(self.lib, stem + "_device")(*head, *[C.c_void_p(d) if d else None for d in device], C.byref(st)))
            return st
        if sink == "rgba8":
            out = np.zeros((rows, width, 4), dtype=np.uint8)
            self._check(getattr(self.lib, stem + "_rgba8")(*head, out.ctypes.data, C.byref(st)))
            return out, st
        if sink == "png":
            params, bound, size, stats = (), lambda: png_bound(width, rows), "png_bytes", PngStats()
            self.png_stats = stats
        elif sink == "jpeg":
            jp = jpeg_params(quality, sampling)
            params, bound, size, stats = (C.byref(jp),), lambda: jpeg_bound(width, rows, quality, sampling), "jpeg_bytes", JpegStats()
            self.jpeg_stats = stats
        else:
            ep = exr_params(pixel)
            params, bound, size, stats = (C.byref(ep),), lambda: exr_bound(width, rows, pixel), "file_bytes", ExrStats()
            self.exr_stats = stats
        cap = bound() if cap is None else int(cap)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        self._check(getattr(self.lib, stem + "_" + sink)(*head, *params, out.ctypes.data, cap, C.byref(stats), C.byref(st)))
        return out[:getattr(stats, size)].tobytes(), st

    def render_ao(self, width, height, depth, samples=16, radius=0.0, seed=0, dirs=False, frame_samples=1, **kw):
        """ndt_hip_render_ao: the ambient occlusion of the frame render(**kw) gives -- for every pixel the cosine-weighted share of
        `samples` rays from its primary hit, over the hemisphere of the N-D normal that faces the viewer, that get away (radius 0) or
        meet nothing nearer than `radius`.  Returns the (rows, width) float64 plane, 1.0 = open and where nothing shows; with
        dirs=True (plane, directions), the directions (samples, dims, rows, width) the device used, zero where a pixel sends none.
        kw: as render()'s (row shards, stereo 1 / 2); `samples` here counts AO rays, the frame's own `-n` is frame_samples (the pass is
        the deterministic frame's whatever it is)."""
        p = self.params(width, height, depth, samples=frame_samples, **kw)
        rows = shard_rows(height, p.row_begin, p.row_step)
        ap = ao_params(samples, radius, seed)
        plane = np.zeros((rows, width), dtype=np.float64)
        used = np.zeros((max(int(samples), 0), self._dims(), rows, width), dtype=np.float64) if dirs else None
        st = RenderStats()
        self._check(self.lib.ndt_hip_render_ao(self.ctx, C.byref(p), C.byref(ap), plane.ctypes.data, used.ctypes.data if dirs else None,
                                               C.byref(st)))
        return (plane, used) if dirs else plane

    def ao_device(self, d_planes, d_ao_ptr, width, height, depth, samples=16, radius=0.0, seed=0, d_dirs_ptr=None, **kw):
        """ndt_hip_ao_device: the pass alone, from the device planes `d_planes` names (a dict "id" / "position" / "normal" / "ray_v" of
        raw device pointers: the feature planes of the rows kw selects) into rows * width doubles at `d_ao_ptr` and, unless None,
        samples * dims * rows * width doubles of directions at `d_dirs_ptr`."""
        p = self.params(width, height, depth, **kw)
        ap = ao_params(samples, radius, seed)
        planes = FeaturePlanes(d_planes.get("id"), d_planes.get("position"), d_planes.get("normal"), None, d_planes.get("ray_v"))
        self._check(self.lib.ndt_hip_ao_device(self.ctx, C.byref(p), C.byref(planes), C.byref(ap), C.c_void_p(d_ao_ptr),
                                               C.c_void_p(d_dirs_ptr) if d_dirs_ptr else None))

    def ao_apply_device(self, d_rgba_in_ptr, d_ao_ptr, n_pixels, strength=1.0, d_rgba_out_ptr=None):
        """ndt_hip_ao_apply_device: rgb * ((1 - strength) + strength * ao) on n_pixels x 4 device doubles, the alpha copied, into
        `d_rgba_out_ptr` (default: in place)."""
        out = d_rgba_in_ptr if d_rgba_out_ptr is None else d_rgba_out_ptr
        self._check(self.lib.ndt_hip_ao_apply_device(self.ctx, C.c_void_p(d_rgba_in_ptr), C.c_void_p(d_ao_ptr), int(n_pixels), float(strength),
                                                     C.c_void_p(out)))

    def ao_launches(self):
        """ndt_hip_ao_launches: kernel launches of the context's last ambient-occlusion call."""
        return int(self.lib.ndt_hip_ao_launches(self.ctx))

    def ao_ms(self):
        """ndt_hip_ao_ms: device time of its pass."""
        return float(self.lib.ndt_hip_ao_ms(self.ctx))

    def render_ao_shaded(self, width, height, depth, sink=None, samples=16, radius=0.0, seed=0, strength=1.0, d_rgba_ptr=None, d_ao_ptr=None,
                         quality=95, sampling="420", cap=None, frame_samples=1, **kw):
        """ndt_hip_render_ao_shaded*: the frame render(samples=frame_samples, **kw) gives, its colour multiplied by (1 - strength) +
        strength * ao, the ambient occlusion of `samples` rays a pixel.  sink
        None: ((rows, width, 4) float64, the (rows, width) plane, RenderStats); "device": left at raw device pointers `d_rgba_ptr`
        (and the plane at `d_ao_ptr` unless None), returns the stats; "rgba8": the (rows, width, 4) uint8 image; "png" / "jpeg":
        the file's bytes (self.png_stats / jpeg_stats keep the record) -- each with the stats."""
        p = self.params(width, height, depth, samples=frame_samples, **kw)
        rows = shard_rows(height, p.row_begin, p.row_step)
        ap = ao_params(samples, radius, seed, strength)
        plane = (np.zeros((rows, width), dtype=np.float64),) if sink is None else ()
        return self._staged_sink("ndt_hip_render_ao_shaded", (self.ctx, C.byref(p), C.byref(ap)), sink, (None, "device", "rgba8", "png", "jpeg"),
                                 rows, width, device=(d_rgba_ptr, d_ao_ptr), extra=plane, quality=quality, sampling=sampling, cap=cap)

    def apng_begin(self, width, rows, n_frames, delay_num=1, delay_den=24, n_plays=0):
        """ndt_hip_apng_begin: opens the context's animated-PNG session: n_frames frames of width x rows pixels are to come, each
        shown delay_num / delay_den seconds, played n_plays times (0: for ever)."""
        self._check(self.lib.ndt_hip_apng_begin(self.ctx, int(width), int(rows), int(n_frames), int(delay_num), int(delay_den), int(n_plays)))
        self._apng_size = (int(width), int(rows))
        self.apng_stats = ApngStats()

    _apng_size = (1, 1)             # before the first apng_begin: room enough for the library to say that no session is open

    def _apng_room(self, cap):
        cap = apng_bound(*self._apng_size) if cap is None else int(cap)
        self.apng_stats = ApngStats()
        return np.zeros(max(cap, 1), dtype=np.uint8), cap

    def apng_add(self, rgba8, cap=None):
        """ndt_hip_apng_add: the session's next frame from a (rows, width, 4) uint8 host image.  Returns the bytes to append to the
        file; self.apng_stats keeps the ndt_apng_stats.  cap: room offered (default: ndt_hip_apng_bound)."""
        rgba8 = np.ascontiguousarray(rgba8, dtype=np.uint8)
        if rgba8.shape != (self._apng_size[1], self._apng_size[0], 4):
            raise ValueError("a frame of shape %r for a session of %d x %d pixels" % ((rgba8.shape,) + self._apng_size))
        out, cap = self._apng_room(cap)
        self._check(self.lib.ndt_hip_apng_add(self.ctx, rgba8.ctypes.data, out.ctypes.data, cap, C.byref(self.apng_stats)))
        return out[:self.apng_stats.bytes].tobytes()

    def apng_add_device(self, d_rgba8_ptr, cap=None):
        """ndt_hip_apng_add_device: the same for the session's width * rows * 4 bytes at raw device pointer `d_rgba8_ptr`."""
        out, cap = self._apng_room(cap)
        self._check(self.lib.ndt_hip_apng_add_device(self.ctx, C.c_void_p(d_rgba8_ptr), out.ctypes.data, cap, C.byref(self.apng_stats)))
        return out[:self.apng_stats.bytes].tobytes()

    def render_apng_frame(self, width, height, depth, ssaa=1, cap=None, **kw):
        """ndt_hip_render_apng_frame: renders the uploaded scene's shard (ssaa 2 .. 8: supersampled) and adds it to the session
        from device memory.  Returns (the bytes to append, RenderStats); self.apng_stats keeps the ndt_apng_stats."""
        p = self.params(width, height, depth, **kw)
        out, cap = self._apng_room(cap)
        st = RenderStats()
        self._check(self.lib.ndt_hip_render_apng_frame(self.ctx, C.byref(p), int(ssaa), out.ctypes.data, cap, C.byref(self.apng_stats),
                                                       C.byref(st)))
        return out[:self.apng_stats.bytes].tobytes(), st

    def apng_end(self):
        """ndt_hip_apng_end: the file's last bytes (IEND) after the session's last frame; closes the session."""
        out, n = np.zeros(16, dtype=np.uint8), C.c_int64(0)
        self._check(self.lib.ndt_hip_apng_end(self.ctx, out.ctypes.data, out.size, C.byref(n)))
        return out[:n.value].tobytes()

    def encode_jpeg(self, rgba8, quality=95, sampling="420", cap=None):
        """ndt_hip_encode_jpeg: the complete baseline JFIF file of a (rows, width, 4) uint8 host image (alpha ignored), made on
        this context's GPU.  Returns the file's bytes; self.jpeg_stats keeps the ndt_jpeg_stats.  cap: room offered (default:
        ndt_hip_jpeg_bound)."""
        rgba8 = np.ascontiguousarray(rgba8, dtype=np.uint8)
        if rgba8.ndim != 3 or rgba8.shape[2] != 4:
            raise ValueError("rgba8 must be (rows, width, 4)")
        rows, width = rgba8.shape[:2]
        jp = jpeg_params(quality, sampling)
        cap = jpeg_bound(width, rows, quality, sampling) if cap is None else int(cap)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        self.jpeg_stats = JpegStats()
        self._check(self.lib.ndt_hip_encode_jpeg(self.ctx, rgba8.ctypes.data, width, rows, C.byref(jp), out.ctypes.data, cap,
                                                 C.byref(self.jpeg_stats)))
        return out[:self.jpeg_stats.jpeg_bytes].tobytes()

    def encode_jpeg_device(self, d_rgba8_ptr, width, rows, quality=95, sampling="420", cap=None):
        """ndt_hip_encode_jpeg_device: the same for width * rows * 4 bytes at raw device pointer `d_rgba8_ptr`."""
        jp = jpeg_params(quality, sampling)
        cap = jpeg_bound(width, rows, quality, sampling) if cap is None else int(cap)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        self.jpeg_stats = JpegStats()
        self._check(self.lib.ndt_hip_encode_jpeg_device(self.ctx, C.c_void_p(d_rgba8_ptr), int(width), int(rows), C.byref(jp),
                                                        out.ctypes.data, cap, C.byref(self.jpeg_stats)))
        return out[:self.jpeg_stats.jpeg_bytes].tobytes()

    def render_jpeg(self, width, height, depth, quality=95, sampling="420", **kw):
        """ndt_hip_render_jpeg: render_rgba8 with the device's JPEG encoder in place of the download.  Returns (the file's bytes,
        RenderStats); self.jpeg_stats keeps the ndt_jpeg_stats.  The file's height is the row shard's."""
        p = self.params(width, height, depth, **kw)
        rows = shard_rows(height, p.row_begin, p.row_step)
        jp = jpeg_params(quality, sampling)
        cap = jpeg_bound(width, rows, quality, sampling)
        out = np.zeros(cap, dtype=np.uint8)
        st = RenderStats()
        self.jpeg_stats = JpegStats()
        self._check(self.lib.ndt_hip_render_jpeg(self.ctx, C.byref(p), C.byref(jp), out.ctypes.data, cap, C.byref(self.jpeg_stats), C.byref(st)))
        return out[:self.jpeg_stats.jpeg_bytes].tobytes(), st

    def depth_rgba8_device(self, d_depth_ptr, n_pixels, d_rgba8_ptr):
        """ndt_hip_depth_rgba8_device: the map of n_pixels doubles at raw device pointer `d_depth_ptr` stretched to 0 .. 1 and
        quantised into n_pixels * 4 bytes at `d_rgba8_ptr` (g, g, g, 255), in two launches.  Returns the map's (lo, hi)."""
        rng = np.zeros(2, dtype=np.float64)
        self._check(self.lib.ndt_hip_depth_rgba8_device(self.ctx, C.c_void_p(d_depth_ptr), int(n_pixels), C.c_void_p(d_rgba8_ptr),
                                                        rng.ctypes.data))
        return rng

    def depth_launches(self):
        """ndt_hip_depth_launches: kernel launches of the context's last depth map."""
        return int(self.lib.ndt_hip_depth_launches(self.ctx))

    def render_rgba8_depth(self, width, height, depth, **kw):
        """ndt_hip_render_rgba8_depth: render_rgba8 with the `-z` map beside it, both finished on the device.  Returns
        ((rows, width, 4) uint8 image, (rows, width, 4) uint8 map, float64 [lo, hi] of the map, RenderStats)."""
        p = self.params(width, height, depth, **kw)
        rows = shard_rows(height, p.row_begin, p.row_step)
        out = np.zeros((rows, width, 4), dtype=np.uint8)
        dm = np.zeros((rows, width, 4), dtype=np.uint8)
        rng = np.zeros(2, dtype=np.float64)
        st = RenderStats()
        self._check(self.lib.ndt_hip_render_rgba8_depth(self.ctx, C.byref(p), out.ctypes.data, dm.ctypes.data, rng.ctypes.data, C.byref(st)))
        return out, dm, rng, st

    def render_png_depth(self, width, height, depth, depth_png=True, cap=None, depth_cap=None, **kw):
        """ndt_hip_render_png_depth: the image as a PNG file made on the device, and the map as one too (depth_png=True) or
        as its (rows, width, 4) bytes.  Returns (file, file or array, [lo, hi], RenderStats); self.png_stats keeps the two
        ndt_png_stats (image, map).  cap / depth_cap: room offered (default: ndt_hip_png_bound)."""
        p = self.params(width, height, depth, **kw)
        rows = shard_rows(height, p.row_begin, p.row_step)
        cap = png_bound(width, rows) if cap is None else int(cap)
        depth_cap = png_bound(width, rows) if depth_cap is None else int(depth_cap)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        dpng = np.zeros(max(depth_cap, 1), dtype=np.uint8) if depth_png else None
        dm = None if depth_png else np.zeros((rows, width, 4), dtype=np.uint8)
        rng = np.zeros(2, dtype=np.float64)
        st = RenderStats()
        self.png_stats = (PngStats * 2)()
        self._check(self.lib.ndt_hip_render_png_depth(self.ctx, C.byref(p), out.ctypes.data, cap, dpng.ctypes.data if depth_png else None,
                                                      depth_cap, None if depth_png else dm.ctypes.data, C.byref(self.png_stats),
                                                      rng.ctypes.data, C.byref(st)))
        png = out[:self.png_stats[0].png_bytes].tobytes()
        return png, (dpng[:self.png_stats[1].png_bytes].tobytes() if depth_png else dm), rng, st

    def ssaa_fold_device(self, d_pass_ptr, d_acc_ptr, width_out, rows, k, a, d_rgba8_ptr=None):
        """ndt_hip_ssaa_fold_device: sub-row `a` of a k x k supersampled frame (rows x k * width_out x 4 doubles at raw device
        pointer `d_pass_ptr`) folded into the rows x width_out x 4 doubles at `d_acc_ptr`; the last step (a = k - 1) divides by
        k * k and, with `d_rgba8_ptr`, writes the 8-bit image there."""
        self._check(self.lib.ndt_hip_ssaa_fold_device(self.ctx, C.c_void_p(d_pass_ptr), C.c_void_p(d_acc_ptr), int(width_out), int(rows),
                                                      int(k), int(a), C.c_void_p(d_rgba8_ptr) if d_rgba8_ptr else None))

    def ssaa_launches(self):
        """ndt_hip_ssaa_launches: fold launches of the context's last supersampled frame."""
        return int(self.lib.ndt_hip_ssaa_launches(self.ctx))

    def ssaa_ms(self):
        """ndt_hip_ssaa_ms: summed device time of those launches."""
        return float(self.lib.ndt_hip_ssaa_ms(self.ctx))

    def _ssaa_params(self, width, height, depth, kw):
        for name in ("aa", "depth_map"):
            if kw.get(name):
                raise ValueError("ssaa is not combined with %s here" % name)
        kw = {k: v for k, v in kw.items() if k not in ("aa", "depth_map")}
        p = self.params(width, height, depth, **kw)
        return p, shard_rows(height, p.row_begin, p.row_step)

    def render_ssaa(self, width, height, depth, ssaa, depth_map=False, **kw):
        """ndt_hip_render_ssaa: the width x height frame supersampled ssaa x ssaa on the device (a box filter in linear light over
        the ssaa * width x ssaa * height frame).  Returns ((rows, width, 4) float64, RenderStats), with depth_map=True
        (rgba, (rows, width) map of sub-sample (0, 0), stats)."""
        p, rows = self._ssaa_params(width, height, depth, kw)
        out = np.zeros((rows, width, 4), dtype=np.float64)
        dm = np.zeros((rows, width), dtype=np.float64) if depth_map else None
        st = RenderStats()
        self._check(self.lib.ndt_hip_render_ssaa(self.ctx, C.byref(p), int(ssaa), out.ctypes.data, dm.ctypes.data if depth_map else None,
                                                 C.byref(st)))
        return (out, dm, st) if depth_map else (out, st)

    def render_ssaa_device(self, d_rgba_ptr, width, height, depth, ssaa, d_depth_ptr=None, **kw):
        """ndt_hip_render_ssaa_device: the same, left in HBM at raw device pointers (the image aligned to 16 bytes)."""
        p, _ = self._ssaa_params(width, height, depth, kw)
        st = RenderStats()
        self._check(self.lib.ndt_hip_render_ssaa_device(self.ctx, C.byref(p), int(ssaa), C.c_void_p(d_rgba_ptr),
                                                        C.c_void_p(d_depth_ptr) if d_depth_ptr else None, C.byref(st)))
        return st

    def render_ssaa_rgba8(self, width, height, depth, ssaa, **kw):
        """ndt_hip_render_ssaa_rgba8: the supersampled frame as the bytes the reference stores: ((rows, width, 4) uint8, stats)."""
        p, rows = self._ssaa_params(width, height, depth, kw)
        return self._staged_sink("ndt_hip_render_ssaa", (self.ctx, C.byref(p), int(ssaa)), "rgba8", ("rgba8",), rows, width)

    def render_ssaa_png(self, width, height, depth, ssaa, **kw):
        """ndt_hip_render_ssaa_png: ... as a PNG file made on the device: (the file's bytes, stats); self.png_stats keeps the record."""
        p, rows = self._ssaa_params(width, height, depth, kw)
        return self._staged_sink("ndt_hip_render_ssaa", (self.ctx, C.byref(p), int(ssaa)), "png", ("png",), rows, width)

    def render_ssaa_jpeg(self, width, height, depth, ssaa, quality=95, sampling="420", **kw):
        """ndt_hip_render_ssaa_jpeg: ... as a JPEG file made on the device: (the file's bytes, stats); self.jpeg_stats keeps the record."""
        p, rows = self._ssaa_params(width, height, depth, kw)
        return self._staged_sink("ndt_hip_render_ssaa", (self.ctx, C.byref(p), int(ssaa)), "jpeg", ("jpeg",), rows, width, quality=quality,
                                 sampling=sampling)

    def render_ssaa_rgba8_depth(self, width, height, depth, ssaa, **kw):
        """ndt_hip_render_ssaa_rgba8_depth: the supersampled frame's bytes and its map (sub-sample (0, 0)'s) finished on the device:
        ((rows, width, 4) uint8 image, (rows, width, 4) uint8 map, float64 [lo, hi], stats)."""
        p, rows = self._ssaa_params(width, height, depth, kw)
        out = np.zeros((rows, width, 4), dtype=np.uint8)
        dm = np.zeros((rows, width, 4), dtype=np.uint8)
        rng = np.zeros(2, dtype=np.float64)
        st = RenderStats()
        self._check(self.lib.ndt_hip_render_ssaa_rgba8_depth(self.ctx, C.byref(p), int(ssaa), out.ctypes.data, dm.ctypes.data, rng.ctypes.data,
                                                            C.byref(st)))
        return out, dm, rng, st

    def quantize_device(self, d_rgba_ptr, d_rgba8_ptr, n_pixels):
        self._check(self.lib.ndt_hip_quantize_device(self.ctx, C.c_void_p(d_rgba_ptr), C.c_void_p(d_rgba8_ptr),
                                                     int(n_pixels)))

    def fit_spheres(self, dims, lists):
        """ndt_hip_fit_spheres: bounds_list_optimal (bounding.c:177-240) for every (points [k, dims], radii [k]) pair of `lists`
        on this context's GPU, bit-identical to the host fit.  Returns (centers [n, dims], radii [n])."""
        first, points, radii = pack_point_lists(int(dims), lists)
        centers = np.zeros((len(lists), int(dims)), dtype=np.float64)
        out = np.zeros(len(lists), dtype=np.float64)
        self._check(self.lib.ndt_hip_fit_spheres(self.ctx, int(dims), len(lists), first.ctypes.data, points.ctypes.data,
                                                 radii.ctypes.data, centers.ctypes.data, out.ctypes.data))
        return centers, out

    def fit_launches(self):
        """ndt_hip_fit_launches: kernel launches of the last fit_spheres call."""
        return int(self.lib.ndt_hip_fit_launches(self.ctx))

    def build_kdtree(self, dims, lower, upper, finite):
        """ndt_hip_build_kdtree + ndt_hip_kdtree_fetch: the reference's kd-tree (kd-tree.c:294-477) of the item boxes lower / upper
        [n, dims] on this context's GPU, byte-identical to the host builder's.  Returns (nodes, leaf_refs, inf_refs, bb_lower,
        bb_upper): nodes in preorder with the dtype of FlatKdNode, the rest int32 / float64; self.kd_counts keeps the counts."""
        from .flat_scene import FlatKdNode
        n, lower, upper, finite = pack_boxes(dims, lower, upper, finite)
        counts = KdCounts()
        self._check(self.lib.ndt_hip_build_kdtree(self.ctx, int(dims), n, lower.ctypes.data, upper.ctypes.data, finite.ctypes.data,
                                                  C.addressof(counts)))
        self.kd_counts = counts
        nodes = np.zeros(counts.n_kd_nodes, dtype=np.dtype(FlatKdNode))
        leaf_refs = np.zeros(counts.n_leaf_refs, dtype=np.int32)
        inf_refs = np.zeros(counts.n_inf, dtype=np.int32)
        bb_lower, bb_upper = np.zeros(int(dims)), np.zeros(int(dims))
        # (an empty array's buffer is still a valid address: the library copies nothing into it)
        self._check(self.lib.ndt_hip_kdtree_fetch(self.ctx, nodes.ctypes.data, leaf_refs.ctypes.data, inf_refs.ctypes.data,
                                                  bb_lower.ctypes.data, bb_upper.ctypes.data))
        return nodes, leaf_refs, inf_refs, bb_lower, bb_upper

    def kd_launches(self):
        """ndt_hip_kd_launches: kernel launches of the last build_kdtree call."""
        return int(self.lib.ndt_hip_kd_launches(self.ctx))

    def trace_rays(self, rays):
        """Batch of trace_kd queries; rays: (n, 2*dims+1) = o, v, dist_limit per row."""
        d = self._dims()
        n = rays.shape[0]
        o = np.ascontiguousarray(rays[:, :d], dtype=np.float64)
        v = np.ascontiguousarray(rays[:, d:2 * d], dtype=np.float64)
        lim = np.ascontiguousarray(rays[:, 2 * d], dtype=np.float64)
        obj = np.zeros(n, dtype=np.int32)
        hit = np.zeros((n, d))
        nrm = np.zeros((n, d))
        self._check(self.lib.ndt_hip_trace_rays(self.ctx, n, o.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p),
                                                lim.ctypes.data_as(C.c_void_p), obj.ctypes.data_as(C.c_void_p),
                                                hit.ctypes.data_as(C.c_void_p), nrm.ctypes.data_as(C.c_void_p)))
        return obj, hit, nrm


def render_multi(contexts, width, height, depth, fmt=IMAGE_F64, d_out_ptr=None, **kw):
    """ONE frame over several NdtHip contexts (one per GPU, or several on one GPU) from this one thread:
    ndt_hip_render_multi.  Rows are dealt cyclically like the reference's MPI_MODE_ROW (ndt.c:812-820); every context
    must hold the same uploaded scene.  Returns (image, stats): float64 (rows, width, 4) or uint8 for IMAGE_RGBA8;
    with d_out_ptr (memory of contexts[0]'s device) the image stays there and only the stats come back."""
    first = contexts[0]
    p = first.params(width, height, depth, **kw)
    arr = (C.c_void_p * len(contexts))(*[c.ctx for c in contexts])
    st = RenderStats()
    if d_out_ptr is not None:
        first._check(first.lib.ndt_hip_render_multi_device(arr, len(contexts), C.byref(p), int(fmt), C.c_void_p(d_out_ptr), C.byref(st)))
        return None, st
    rows = shard_rows(height, p.row_begin, p.row_step)
    out = np.zeros((rows, width, 4), dtype=np.uint8 if fmt == IMAGE_RGBA8 else np.float64)
    first._check(first.lib.ndt_hip_render_multi(arr, len(contexts), C.byref(p), int(fmt), out.ctypes.data_as(C.c_void_p), C.byref(st)))
    return out, st
