"""ctypes binding of libesahrnet.so (include/esahrnet.h).  No torch types cross this boundary:
device buffers are passed as raw pointers (tensor.data_ptr()) and the stream as a hipStream_t."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libesahrnet.so")
MAX_BRANCHES = 4
ABI_VERSION = 6
# a report row of esahrnet_pnp_batch_ex / esahrnet_pnp_batch_w_ex (include/esahrnet.h: enum esahrnet_pose_report)
POSE_REPORT_FIELDS = ("status", "flags", "n", "inliers", "ransac_iters", "lm_iters", "cost", "rms_px", "max_px", "argmax",
                      "min_depth", "s2")
POSE_REPORT_COV = 12
POSE_REPORT_DOUBLES = 33
MAX_CANDIDATES = 4                # ESAHRNET_MAX_CANDIDATES: peaks per heat-map esahrnet_keypoints_candidates keeps at most


class Cfg(C.Structure):
    _fields_ = [("cin", C.c_int32), ("num_keypoints", C.c_int32), ("stem_width", C.c_int32),
                ("widths", C.c_int32 * MAX_BRANCHES), ("blocks", (C.c_int32 * MAX_BRANCHES) * 4),
                ("modules", C.c_int32 * 4), ("final_conv_kernel", C.c_int32), ("variant", C.c_int32),
                ("precision", C.c_int32)]


class AuxDesc(C.Structure):
    _fields_ = [("name", C.c_char * 96), ("shape", C.c_int32 * 4)]


class ConvDesc(C.Structure):
    _fields_ = [("name", C.c_char * 96), ("bn", C.c_char * 96), ("cin", C.c_int32),
                ("cout", C.c_int32), ("k", C.c_int32), ("stride", C.c_int32),
                ("has_bias", C.c_int32), ("relu", C.c_int32)]


class OpDesc(C.Structure):
    _fields_ = [("kernel", C.c_char * 64), ("label", C.c_char * 96), ("flops", C.c_double),
                ("bytes", C.c_double)]


class DebugRegion(C.Structure):
    _fields_ = [("tensor", C.c_int32), ("role", C.c_int32), ("write", C.c_int32), ("slice", C.c_int32),
                ("offset", C.c_uint64), ("bytes", C.c_uint64)]


class DebugOp(C.Structure):
    _fields_ = [("index", C.c_int32), ("wave", C.c_int32), ("lane", C.c_int32), ("job", C.c_int32), ("multi", C.c_int32),
                ("nregions", C.c_int32), ("regions", DebugRegion * 8)]


# One record of the activation range report (include/esahrnet.h: ESAHRNET_STATS_FIELDS, the same names in the same order; the
# header test holds the two together).  The ctypes struct and the numpy dtype below both come from this table.
STATS_RECORD_BYTES = 64
STATS_FIELDS = (("sum_abs", "f8"), ("max_abs", "f4"), ("min", "f4"), ("max", "f4"), ("n_finite", "u4"), ("n_nan", "u4"),
                ("n_inf", "u4"), ("n_zero", "u4"), ("n_ge_f16max", "u4"), ("n_f16_tiny", "u4"))
_STATS_CTYPES = {"f8": C.c_double, "f4": C.c_float, "u4": C.c_uint32}
STATS_NCHW = -1                   # esahrnet_stats_row_desc.fmt of the heat-maps row; 0..3: the plan's storage formats
STATS_FORMATS = {0: "bf16x3", 1: "bf16", 2: "f32", 3: "fp16", STATS_NCHW: "f32 NCHW"}


class StatsRecord(C.Structure):
    _fields_ = [(name, _STATS_CTYPES[t]) for name, t in STATS_FIELDS] + [("reserved", C.c_uint32 * 5)]


def stats_dtype():
    """numpy dtype of a record: the fields of STATS_FIELDS at their offsets, 64 bytes."""
    import numpy as np
    names = [name for name, _ in STATS_FIELDS]
    return np.dtype({"names": names, "formats": [t for _, t in STATS_FIELDS],
                     "offsets": [getattr(StatsRecord, name).offset for name in names], "itemsize": STATS_RECORD_BYTES})


class StatsRowDesc(C.Structure):
    _fields_ = [("name", C.c_char * 96), ("def_op", C.c_int32), ("c", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("fmt", C.c_int32), ("scanned", C.c_int32)]


# One record of the precision report (include/esahrnet.h: ESAHRNET_DIFF_FIELDS, held together by the header test as above)
DIFF_RECORD_BYTES = 64
DIFF_FIELDS = (("sum_abs_err", "f8"), ("sum_sq_err", "f8"), ("sum_sq_ref", "f8"), ("max_abs_err", "f4"), ("max_abs_ref", "f4"),
               ("max_abs_test", "f4"), ("at", "u4"), ("n_compared", "u4"), ("n_nonfinite_test", "u4"), ("n_nonfinite_ref", "u4"),
               ("n_class_differs", "u4"))
DIFF_AT_NONE = 0xFFFFFFFF         # esahrnet_diff_record.at when nothing was compared


class DiffRecord(C.Structure):
    _fields_ = [(name, _STATS_CTYPES[t]) for name, t in DIFF_FIELDS] + [("reserved", C.c_uint32 * 2)]


def diff_dtype():
    """numpy dtype of a record: the fields of DIFF_FIELDS at their offsets, 64 bytes."""
    import numpy as np
    names = [name for name, _ in DIFF_FIELDS]
    return np.dtype({"names": names, "formats": [t for _, t in DIFF_FIELDS],
                     "offsets": [getattr(DiffRecord, name).offset for name in names], "itemsize": DIFF_RECORD_BYTES})


class DiffRowDesc(C.Structure):
    _fields_ = [("key", C.c_char * 96), ("ref_row", C.c_int32), ("c", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("fmt", C.c_int32), ("ref_fmt", C.c_int32), ("exponent", C.c_int32), ("compared", C.c_int32)]


SCALE_MAX_RANGES = 4              # ESAHRNET_SCALE_MAX_RANGES
SCALE_MAX_EXPONENT = 32           # ESAHRNET_SCALE_MAX_EXPONENT


class ScaleConv(C.Structure):
    _fields_ = [("out_group", C.c_int32), ("nranges", C.c_int32), ("c0", C.c_int32 * SCALE_MAX_RANGES),
                ("c1", C.c_int32 * SCALE_MAX_RANGES), ("in_group", C.c_int32 * SCALE_MAX_RANGES)]


class EsaHrnetError(RuntimeError):
    pass


_lib = None

_SIGS = {
    "esahrnet_last_error": (C.c_char_p, []),
    "esahrnet_abi_version": (C.c_int, []),
    "esahrnet_create": (C.c_int, [C.POINTER(Cfg), C.c_int, C.POINTER(C.c_void_p)]),
    "esahrnet_destroy": (C.c_int, [C.c_void_p]),
    "esahrnet_handle_device": (C.c_int, [C.c_void_p]),
    "esahrnet_debug_devstate": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "esahrnet_debug_set_launch_limit": (C.c_int, [C.c_longlong]),
    "esahrnet_debug_set_x6_grid_limit": (C.c_int, [C.c_int]),
    "esahrnet_debug_op_schedule": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "esahrnet_debug_op_count": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "esahrnet_debug_op_regions": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DebugOp)]),
    "esahrnet_conv_count": (C.c_int, [C.c_void_p]),
    "esahrnet_conv_desc_get": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(ConvDesc)]),
    "esahrnet_set_conv": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "esahrnet_aux_count": (C.c_int, [C.c_void_p]),
    "esahrnet_aux_desc_get": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(AuxDesc)]),
    "esahrnet_set_aux": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "esahrnet_commit": (C.c_int, [C.c_void_p]),
    "esahrnet_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "esahrnet_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_size_t, C.c_void_p]),
    "esahrnet_keypoints": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "esahrnet_keypoints_ex": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "esahrnet_keypoints_final2_workspace_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "esahrnet_keypoints_final2": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_size_t, C.c_void_p]),
    "esahrnet_partial_tiles": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "esahrnet_forward_partials": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_size_t, C.c_void_p]),
    "esahrnet_keypoints_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
    "esahrnet_keypoints_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "esahrnet_forward_keypoints": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_size_t, C.c_void_p]),
    "esahrnet_keypoints_final2_forward_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                                   C.POINTER(C.c_size_t)]),
    "esahrnet_forward_keypoints_final2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_size_t, C.c_void_p]),
    "esahrnet_crops": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float,
                                 C.c_void_p, C.c_void_p]),
    "esahrnet_boxes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p]),
    "esahrnet_crops_ex": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "esahrnet_frames_keypoints_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "esahrnet_frames_keypoints": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "esahrnet_pnp_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "esahrnet_keypoints_final2_hess": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_size_t, C.c_void_p]),
    "esahrnet_forward_keypoints_final2_hess": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                         C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "esahrnet_keypoints_gaussfit": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p]),
    "esahrnet_keypoints_gaussfit_forward_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                                     C.POINTER(C.c_size_t)]),
    "esahrnet_forward_keypoints_gaussfit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "esahrnet_frames_keypoints_gaussfit_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "esahrnet_frames_keypoints_gaussfit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                     C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "esahrnet_keypoints_gaussfit_cov": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]),
    "esahrnet_forward_keypoints_gaussfit_cov": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                                          C.c_void_p, C.c_size_t, C.c_void_p]),
    "esahrnet_frames_keypoints_gaussfit_cov": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                         C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p,
                                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_size_t,
                                                         C.c_void_p]),
    "esahrnet_correspondences": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double,
                                           C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "esahrnet_frames_correspondences_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                                  C.POINTER(C.c_size_t)]),
    "esahrnet_frames_correspondences": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                  C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_double,
                                                  C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                  C.c_void_p]),
    "esahrnet_pnp_batch_w": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_int, C.c_void_p, C.c_void_p]),
    "esahrnet_pnp_batch_ex": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "esahrnet_pnp_batch_w_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "esahrnet_keypoints_candidates": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                C.c_void_p, C.c_void_p]),
    "esahrnet_keypoints_candidates_form": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "esahrnet_keypoints_candidates_forward_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                                       C.POINTER(C.c_size_t)]),
    "esahrnet_forward_keypoints_candidates": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "esahrnet_frames_keypoints_candidates_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "esahrnet_frames_keypoints_candidates": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                       C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int,
                                                       C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_size_t, C.c_void_p]),
    "esahrnet_pnp_batch_cand": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_double, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "esahrnet_keypoints_at_workspace_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "esahrnet_keypoints_at": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                                        C.c_size_t, C.c_void_p]),
    "esahrnet_keypoints_candidates_refined": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.c_double, C.c_void_p, C.c_size_t, C.c_void_p]),
    "esahrnet_keypoints_candidates_refined_forward_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                                               C.POINTER(C.c_size_t)]),
    "esahrnet_forward_keypoints_candidates_refined": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                                C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                                C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_size_t,
                                                                C.c_void_p]),
    "esahrnet_frames_keypoints_candidates_refined_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                                              C.POINTER(C.c_size_t)]),
    "esahrnet_frames_keypoints_candidates_refined": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                               C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int,
                                                               C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p,
                                                               C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "esahrnet_pnp_batch_cand_w": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_double, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
    "esahrnet_correspondences_cand": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p]),
    "esahrnet_pnp_batch_cand_pts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p]),
    "esahrnet_gather_records": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p]),
    "esahrnet_flops_per_crop": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "esahrnet_launch_count": (C.c_int, [C.c_void_p]),
    "esahrnet_op_desc_get": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(OpDesc)]),
    "esahrnet_forward_timed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_float)]),
    "esahrnet_tap_count": (C.c_int, [C.c_void_p]),
    "esahrnet_tap_name": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t]),
    "esahrnet_set_debug_keep": (C.c_int, [C.c_void_p, C.c_int]),
    "esahrnet_tap_shape": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_int),
                                     C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "esahrnet_tap_read": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "esahrnet_stats_rows": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "esahrnet_stats_row_get": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(StatsRowDesc)]),
    "esahrnet_forward_stats_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "esahrnet_forward_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.c_void_p, C.c_void_p]),
    "esahrnet_forward_stats_h0_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "esahrnet_forward_stats_h0": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "esahrnet_scale_groups": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "esahrnet_scale_group_name": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t]),
    "esahrnet_scale_conv_get": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(ScaleConv)]),
    "esahrnet_scale_row_group": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "esahrnet_set_scale_exponents": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    "esahrnet_get_scale_exponents": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    "esahrnet_debug_scaled_conv": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "esahrnet_scale_exponents_from_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                      C.POINTER(C.c_int32), C.c_int]),
    "esahrnet_tensor_stats_workspace_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                       C.POINTER(C.c_size_t)]),
    "esahrnet_tensor_stats": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                        C.c_void_p, C.c_void_p]),
    "esahrnet_tensor_diff_workspace_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                      C.POINTER(C.c_size_t)]),
    "esahrnet_tensor_diff": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "esahrnet_diff_row_get": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DiffRowDesc)]),
    "esahrnet_forward_diff_workspace_bytes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "esahrnet_forward_diff": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "esahrnet_op_conv": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "esahrnet_op_fuse": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                   C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "esahrnet_op_conv_ex": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "esahrnet_op_fuse_ex": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                      C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "esahrnet_op_cbam": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "esahrnet_op_cbam_steps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "esahrnet_op_stem": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]),
    "esahrnet_op_resample": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                       C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "esahrnet_op_zero_slice": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "esahrnet_debug_set_cu_limit": (C.c_int, [C.c_int]),
    "esahrnet_op_conv_kernel": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_char_p, C.c_size_t]),
    "esahrnet_op_conv_group": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                         C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int),
                                         C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                         C.c_int, C.c_char_p, C.c_size_t, C.c_void_p]),
    "esahrnet_op_conv_multi": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_void_p),
                                         C.c_void_p]),
    "esahrnet_op_block32": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "esahrnet_op_stem2": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                    C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    # the stem, the layout conversions and the tile-maximum kernels on their own (tests only)
    "esahrnet_op_stem_ex": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                      C.c_int, C.c_void_p, C.c_void_p]),
    "esahrnet_op_layout": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "esahrnet_op_tile_max": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p]),
}


def exported_symbols():
    """Every entry point include/esahrnet.h declares."""
    return sorted(_SIGS)


def lib():
    """Load libesahrnet.so (built in-tree by build.py).  There is NO fallback: without the HIP
    library the product path does not exist."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EsaHrnetError(
            f"{LIB_PATH} is missing — build it with `python __graft_entry__.py` "
            "(hipcc --offload-arch=gfx950). There is no CPU/PyTorch fallback for this path.")
    # torch's ROCm wheel bundles its own libamdhip64.so.7; the process must have ONE HIP runtime and
    # it has to be the one torch's allocator/streams live in, so torch is loaded first and
    # libesahrnet.so's NEEDED libamdhip64.so.7 then resolves to the already-loaded copy.
    import torch  # noqa: F401
    l = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(l, name)           # AttributeError = header/library mismatch: fail loudly
        fn.restype, fn.argtypes = res, args
    if l.esahrnet_abi_version() != ABI_VERSION:
        raise EsaHrnetError("libesahrnet.so ABI version mismatch — rebuild it")
    _lib = l
    return l


def load_other(path: str):
    """Another build of the library (a measurement against an older libesahrnet.so), bound like lib() with the entries it has.
    For hrnet._Runtime.use_library only; errors of calls through it are read from it, not from lib()."""
    import torch  # noqa: F401
    other = C.CDLL(os.path.abspath(path))
    for name, (res, args) in _SIGS.items():
        if hasattr(other, name):
            fn = getattr(other, name)
            fn.restype, fn.argtypes = res, args
    return other


def check(rc: int):
    if rc != 0:
        raise EsaHrnetError(lib().esahrnet_last_error().decode(errors="replace"))
