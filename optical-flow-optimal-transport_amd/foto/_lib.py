"""ctypes binding of libfoto.so (the C ABI declared in include/foto.h).

This is the only place Python touches the native library.  There is no fallback: if
libfoto.so is missing or cannot be loaded, ``lib()`` raises, and every compute call that
fails on the device raises ``FotoError`` with the library's message.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FOTO_LIB", os.path.join(HERE, "libfoto.so"))

FOTO_ERR_ARG = -1
FOTO_ERR_HIP = -2
FOTO_ERR_COMM = -3
FOTO_ERR_STATE = -4
FOTO_ERR_BC = -5

K_CG_DIR, K_CG_UPD, K_RHS, K_PROX, K_SPEC, K_DCT, K_FLOW, K_SLAB = range(8)
K_OTHER = K_SLAB
# dct_slab: the sharded path's slab-side x / y DCTs (foto.h FOTO_K_SLAB), apart from "dct" (the
# box-side t axis, x^) so the scaling proxy sees what the pipelined all-to-alls overlap
K_NAMES = ["cg_dir", "cg_upd", "rhs", "prox", "spec_cg", "dct", "flow", "dct_slab"]


class FotoError(RuntimeError):
    pass


class BBOpts(ctypes.Structure):
    _fields_ = [
        ("device", ctypes.c_int),
        ("cg_maxiter", ctypes.c_int),
        ("cg_rtol", ctypes.c_double),
        ("cg_mode", ctypes.c_int),
        ("rank", ctypes.c_int),
        ("world", ctypes.c_int),
        ("nccl_id", ctypes.c_void_p),
        ("virtual_ranks", ctypes.c_int),
        ("timing", ctypes.c_int),
    ]


class BBStats(ctypes.Structure):
    _fields_ = [
        ("outer_iters", ctypes.c_int),
        ("cg_iters_total", ctypes.c_int64),
        ("last_crit", ctypes.c_double),
        ("ms_rhs", ctypes.c_double),
        ("ms_cg", ctypes.c_double),
        ("ms_prox", ctypes.c_double),
        ("ms_flow", ctypes.c_double),
        ("n_k", ctypes.c_int64 * 8),
        ("ms_k", ctypes.c_double * 8),
        ("bytes_k", ctypes.c_double * 8),
        ("cg_redo", ctypes.c_int),
    ]


class BBSolveStats(ctypes.Structure):
    """foto_bb_solve_stats (include/foto.h): the caller sizes crit / cg_its / cg_info by cap."""
    _fields_ = [
        ("cap", ctypes.c_int),
        ("crit", ctypes.POINTER(ctypes.c_double)),
        ("cg_its", ctypes.POINTER(ctypes.c_int)),
        ("cg_info", ctypes.POINTER(ctypes.c_int)),
        ("outer_iters", ctypes.c_int),
        ("stopped", ctypes.c_int),
        ("phi_t0", ctypes.c_int),
        ("phi_nloc", ctypes.c_int),
        ("ms_create", ctypes.c_double),
        ("ms_loop", ctypes.c_double),
        ("ms_flow", ctypes.c_double),
        ("alg_bytes_per_iter", ctypes.c_double),
        ("bb", BBStats),
    ]


class GNStats(ctypes.Structure):
    """foto_gn_stats (include/foto.h)."""
    _fields_ = [
        ("iterations", ctypes.c_int),
        ("info", ctypes.c_int),
        ("plan_reused", ctypes.c_int),
        ("levels", ctypes.c_int),
        ("ms_setup", ctypes.c_double),
        ("ms_pcg", ctypes.c_double),
        ("ms_total", ctypes.c_double),
        ("alg_bytes_per_iter", ctypes.c_double),
    ]


GN_PYR_MAX_LEVELS = 16


class GNPyrOpts(ctypes.Structure):
    """foto_gn_pyr_opts (include/foto.h)."""
    _fields_ = [
        ("levels", ctypes.c_int),
        ("warps", ctypes.c_int),
        ("min_size", ctypes.c_int),
        ("rtol", ctypes.c_double),
        ("maxiter", ctypes.c_int),
    ]


class GNPyrStats(ctypes.Structure):
    """foto_gn_pyr_stats (include/foto.h): the caller sizes its / info by cap."""
    _fields_ = [
        ("cap", ctypes.c_int),
        ("its", ctypes.POINTER(ctypes.c_int)),
        ("info", ctypes.POINTER(ctypes.c_int)),
        ("levels", ctypes.c_int),
        ("solves", ctypes.c_int),
        ("wl", ctypes.c_int * GN_PYR_MAX_LEVELS),
        ("hl", ctypes.c_int * GN_PYR_MAX_LEVELS),
        ("ms_level", ctypes.c_double * GN_PYR_MAX_LEVELS),
        ("ms_new", ctypes.c_double),
        ("ms_total", ctypes.c_double),
    ]


class TVL1Opts(ctypes.Structure):
    """foto_tvl1_opts (include/foto.h)."""
    _fields_ = [
        ("lam", ctypes.c_double),   # (`lambda` in C)
        ("theta", ctypes.c_double),
        ("tau", ctypes.c_double),
        ("gamma", ctypes.c_double),
        ("levels", ctypes.c_int),
        ("warps", ctypes.c_int),
        ("iters", ctypes.c_int),
        ("min_size", ctypes.c_int),
        ("per_launch", ctypes.c_int),
    ]


FOTO_TVL1_MAX_PER_LAUNCH = 8


class TVL1Stats(ctypes.Structure):
    """foto_tvl1_stats (include/foto.h): the caller sizes the four arrays by cap."""
    _fields_ = [
        ("cap", ctypes.c_int),
        ("wl", ctypes.POINTER(ctypes.c_int)),
        ("hl", ctypes.POINTER(ctypes.c_int)),
        ("launches", ctypes.POINTER(ctypes.c_int)),
        ("ms_level", ctypes.POINTER(ctypes.c_double)),
        ("levels", ctypes.c_int),
        ("launches_total", ctypes.c_int),
        ("ms_total", ctypes.c_double),
    ]


FOTO_U8, FOTO_F32, FOTO_F64 = 0, 1, 2
FOTO_INV_ITERS_MAX, FOTO_INV_ITERS_DEFAULT = 64, 6   # (include/foto.h, maps and in-betweens)


class Image(ctypes.Structure):
    """foto_image (include/foto.h): a strided device view of one grey-scale frame."""
    _fields_ = [
        ("data", ctypes.c_void_p),
        ("dtype", ctypes.c_int),
        ("stride_y", ctypes.c_int64),
        ("stride_x", ctypes.c_int64),
        ("divisor", ctypes.c_double),
    ]


class Flow(ctypes.Structure):
    """foto_flow (include/foto.h): a device flow buffer as the *_dev entries write it."""
    _fields_ = [
        ("data", ctypes.c_void_p),
        ("dtype", ctypes.c_int),
        ("layout", ctypes.c_int),
        ("records", ctypes.c_int),
    ]


FOTO_SCORE_COLS, FOTO_SCORE_MAX_RECORDS = 32, 65535   # (include/foto.h, scoring)
FOTO_CONSISTENCY_ALPHA1, FOTO_CONSISTENCY_ALPHA2 = 0.01, 0.5   # (include/foto.h, flow algebra)


class ScoreOpts(ctypes.Structure):
    """foto_score_opts (include/foto.h): the cap, thresholds and percentiles of a flow score."""
    _fields_ = [
        ("ee_cap", ctypes.c_double),
        ("n_ee_thr", ctypes.c_int),
        ("n_ae_thr", ctypes.c_int),
        ("n_pct", ctypes.c_int),
        ("reserved", ctypes.c_int),
        ("ee_thr", ctypes.c_double * 4),
        ("ae_thr", ctypes.c_double * 4),
        ("pct", ctypes.c_double * 4),
    ]


# (include/foto.h, flow filtering)
FOTO_MEDIAN_MAX_RADIUS, FOTO_MEDIAN_MAX_ROUNDS, FOTO_MEDIAN_MAX_RANGE = 7, 64, 256
FOTO_MEDIAN_TILE_W, FOTO_MEDIAN_TILE_H = 32, 8   # the kernel's tile: the tests' frame sizes derive from it


class MedianOpts(ctypes.Structure):
    """foto_median_opts (include/foto.h): radius, rounds and the two integer weight tables of the
    weighted median."""
    _fields_ = [
        ("radius", ctypes.c_int),
        ("rounds", ctypes.c_int),
        ("fill_only", ctypes.c_int),
        ("n_range", ctypes.c_int),
        ("range_scale", ctypes.c_double),
        ("spatial", ctypes.c_uint16 * (15 * 15)),
        ("range", ctypes.c_uint16 * 256),
    ]


# (include/foto.h, frame preparation)
FOTO_FILTER_BOX, FOTO_FILTER_BILINEAR, FOTO_FILTER_BICUBIC, FOTO_FILTER_LANCZOS = range(4)
FOTO_PREP_TILE_X, FOTO_PREP_MAX_SHAPES, FOTO_RESIZE_MAX_TABLE = 64, 8, 1 << 22
FOTO_RESIZE_ROUTE_AUTO, FOTO_RESIZE_ROUTE_LDS, FOTO_RESIZE_ROUTE_DIRECT = range(3)
FOTO_LUM_RECT, FOTO_LUM_CIRCLE = 0, 1


class LumShape(ctypes.Structure):
    """foto_lum_shape (include/foto.h): one rectangle or disc of added illumination."""
    _fields_ = [
        ("kind", ctypes.c_int),
        ("reserved", ctypes.c_int),
        ("p", ctypes.c_double * 4),
        ("v", ctypes.c_double),
    ]


# (include/foto.h, sparse tracking)
FOTO_CORNER_MAX_WINDOW, FOTO_CORNER_MAX_NMS, FOTO_LK_MAX_RADIUS = 7, 15, 7
FOTO_LK_FLAT, FOTO_LK_OUT, FOTO_LK_NONFINITE, FOTO_LK_INCONSISTENT = 1, 2, 4, 8


class CornerOpts(ctypes.Structure):
    """foto_corner_opts (include/foto.h): the Shi-Tomasi detector's quality, box radius, suppression
    radius and margin."""
    _fields_ = [
        ("quality", ctypes.c_double),
        ("window", ctypes.c_int),
        ("nms", ctypes.c_int),
        ("margin", ctypes.c_int),
        ("reserved", ctypes.c_int),
    ]


class LKOpts(ctypes.Structure):
    """foto_lk_opts (include/foto.h): the Lucas-Kanade window radius, pyramid and fixed counts."""
    _fields_ = [
        ("radius", ctypes.c_int),
        ("levels", ctypes.c_int),
        ("min_size", ctypes.c_int),
        ("iters", ctypes.c_int),
        ("min_eig", ctypes.c_double),
    ]


# (include/foto.h, global motion)
FOTO_MOTION_TRANSLATION, FOTO_MOTION_SIMILARITY, FOTO_MOTION_AFFINE, FOTO_MOTION_HOMOGRAPHY = range(4)
FOTO_MOTION_NONE, FOTO_MOTION_KEPT, FOTO_MOTION_TILE = 1, 2, 1024


class MotionOpts(ctypes.Structure):
    """foto_motion_opts (include/foto.h): the model, the refinement rounds, the inlier bar and the
    inlier distance of a global-motion fit."""
    _fields_ = [
        ("model", ctypes.c_int),
        ("rounds", ctypes.c_int),
        ("min_inliers", ctypes.c_int),
        ("reserved", ctypes.c_int),
        ("threshold", ctypes.c_double),
    ]


# (include/foto.h, feature matching)
FOTO_MATCH_MAX_PATCH, FOTO_MATCH_MAX_ORIENT, FOTO_MATCH_MAX_BLUR = 31, 32, 7
FOTO_MATCH_NONE, FOTO_MATCH_OUT, FOTO_MATCH_NONFINITE, FOTO_MATCH_NOT_MUTUAL, FOTO_MATCH_AMBIGUOUS = 1, 2, 4, 8, 16
FOTO_MATCH_TILE, FOTO_MATCH_QUERIES, FOTO_MATCH_BLOCKS = 256, 512, 1024   # the matcher's shape: the tests' sizes


class DescribeOpts(ctypes.Structure):
    """foto_describe_opts (include/foto.h): the box radius, the disc's radius and the orientation bins."""
    _fields_ = [
        ("blur", ctypes.c_int),
        ("patch", ctypes.c_int),
        ("orientations", ctypes.c_int),
        ("reserved", ctypes.c_int),
    ]


class MatchOpts(ctypes.Structure):
    """foto_match_opts (include/foto.h): the spatial gate, the distance bound and Lowe's ratio in 1 / 256."""
    _fields_ = [
        ("max_disp", ctypes.c_double),
        ("max_dist", ctypes.c_int),
        ("ratio", ctypes.c_int),
        ("reserved", ctypes.c_int * 2),
    ]


# (include/foto.h, entropic transport)
FOTO_SINKHORN_MAX_RADIUS, FOTO_SINKHORN_TILE_W, FOTO_SINKHORN_TILE_H = 32, 64, 32


class SinkhornOpts(ctypes.Structure):
    """foto_sinkhorn_opts (include/foto.h): the window radius and the kernel's variance."""
    _fields_ = [
        ("radius", ctypes.c_int),
        ("per_launch_reserved", ctypes.c_int),
        ("eps", ctypes.c_double),
    ]


ITER_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int)

_D = ctypes.POINTER(ctypes.c_double)
_I = ctypes.c_int
_Dbl = ctypes.c_double
_P = ctypes.c_void_p

# name -> (restype, argtypes)
SIGNATURES = {
    "foto_last_error": (ctypes.c_char_p, []),
    "foto_version": (_I, []),
    "foto_device_count": (_I, [ctypes.POINTER(_I)]),
    "foto_grad_st": (_I, [_D, _I, _I, _I, _D]),
    "foto_div_st": (_I, [_D, _I, _I, _I, _D]),
    "foto_laplacian_st": (_I, [_D, _I, _I, _I, _D]),
    "foto_apply_A": (_I, [_D, _I, _I, _I, _Dbl, _Dbl, _D]),
    "foto_grad2": (_I, [_D, _I, _I, ctypes.c_char, _D]),
    "foto_div2": (_I, [_D, _I, _I, ctypes.c_char, _D]),
    "foto_grad2_forward": (_I, [_D, _I, _I, _D]),
    "foto_stepB": (_I, [_D, ctypes.c_int64, _D]),
    "foto_bb_rhs": (_I, [_D, _D, _D, _D, _I, _I, _I, _Dbl, _D]),
    "foto_cg": (_I, [_D, _I, _I, _I, _Dbl, _Dbl, _Dbl, _I, _I, _D, ctypes.POINTER(_I)]),
    "foto_flow_from_phi": (_I, [_D, _I, _I, _I, _D, _D, _D]),
    "foto_bb_opts_default": (_I, [ctypes.POINTER(BBOpts)]),
    "foto_bb_create": (_I, [_D, _D, _I, _I, _I, _Dbl, _Dbl, ctypes.POINTER(BBOpts), ctypes.POINTER(_P)]),
    "foto_bb_iterate": (_I, [_P, _I, _Dbl, _I, ITER_CB, _P, ctypes.POINTER(_I)]),
    "foto_bb_flow": (_I, [_P, _D, _D, _D]),
    "foto_bb_reset": (_I, [_P, _D, _D]),
    "foto_bb_get_phi": (_I, [_P, _D]),
    "foto_bb_get_state": (_I, [_P, _D, _D]),
    "foto_bb_shard": (_I, [_P, ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "foto_bb_comm_size": (_I, [_P, ctypes.POINTER(_I)]),
    "foto_bb_stats_get": (_I, [_P, ctypes.POINTER(BBStats)]),
    "foto_bb_stats_reset": (_I, [_P]),
    "foto_bb_set_timing": (_I, [_P, _I]),
    "foto_bb_sync": (_I, [_P]),
    "foto_bb_destroy": (None, [_P]),
    "foto_bb_solve": (_I, [_D, _D, _I, _I, _I, _Dbl, _Dbl, _Dbl, _I, ITER_CB, _P, _D, _D, _D]),
    "foto_bb_solve_ex": (_I, [_D, _D, _I, _I, _I, _Dbl, _Dbl, _Dbl, _I, ctypes.POINTER(BBOpts), _D, _D, _D, _D,
                              ctypes.POINTER(BBSolveStats)]),
    "foto_nccl_unique_id": (_I, [_P]),
    "foto_xfer_calls": (_I, [_I, _I, _I, _I, _I, _I, _I, ctypes.POINTER(ctypes.c_int64), _I, ctypes.POINTER(_I)]),
    "foto_dct": (_I, [_D, _I, _I, _I, _I, _I, _D]),
    "foto_stream_probe": (_I, [ctypes.c_int64, _I, _D]),
    "foto_stream_probe4": (_I, [ctypes.c_int64, _I, _D]),
    "foto_gn_apply": (_I, [_D, _D, _I, _I, _Dbl, _Dbl, _D, _D]),
    "foto_gn_rhs": (_I, [_D, _D, _I, _I, _D]),
    "foto_gn_solve": (_I, [_D, _D, _I, _I, _Dbl, _Dbl, _Dbl, _I, _D, _D, _D, ctypes.POINTER(_I)]),
    "foto_gn_solve_ex": (_I, [_D, _D, _I, _I, _Dbl, _Dbl, _Dbl, _I, _D, _D, _D, ctypes.POINTER(GNStats)]),
    "foto_gn_plan_create": (_I, [_I, _I, _Dbl, _Dbl, _Dbl, _I, ctypes.POINTER(_P)]),
    "foto_gn_plan_solve": (_I, [_P, _D, _D, _D, _D, _D, ctypes.POINTER(_I)]),
    "foto_gn_plan_timing": (_I, [_P, _D]),
    "foto_gn_plan_device": (_I, [_P]),
    "foto_gn_plan_destroy": (None, [_P]),
    "foto_warp": (_I, [_D, _D, _D, _D, _I, _I, _D]),
    "foto_flow_errors": (_I, [_D, _D, _D, _D, _I, _I, _D]),
    "foto_intensity_error": (_I, [_D, _D, _I, _I, _D]),
    # device buffers (device pointers travel as void*)
    "foto_image_check": (_I, [ctypes.POINTER(Image), _I, _I]),
    "foto_bb_create_dev": (_I, [ctypes.POINTER(Image), ctypes.POINTER(Image), _I, _P, _I, _I, _I, _Dbl, _Dbl,
                                ctypes.POINTER(BBOpts), _D, ctypes.POINTER(_P)]),
    "foto_bb_reset_dev": (_I, [_P, ctypes.POINTER(Image), ctypes.POINTER(Image), _I, _P, _D]),
    "foto_bb_flow_dev": (_I, [_P, _P, _I, _I, _P]),
    # the transport path: density frames and the Nt - 1 partial flows
    "foto_flow_path_from_phi": (_I, [_D, _I, _I, _I, _D, _D, _D]),
    "foto_bb_frames": (_I, [_P, _D, _I, _Dbl, _D]),
    "foto_bb_frames_dev": (_I, [_P, _D, _I, _Dbl, _P, _I, _P]),
    "foto_bb_flow_path": (_I, [_P, _D, _D, _D]),
    "foto_bb_flow_path_dev": (_I, [_P, _P, _I, _I, _P]),
    # point tracking: trajectories from arbitrary start points
    "foto_track_from_phi": (_I, [_D, _I, _I, _I, _D, ctypes.c_int64, _I, _D]),
    "foto_bb_track": (_I, [_P, _D, ctypes.c_int64, _I, _D]),
    "foto_bb_track_dev": (_I, [_P, _P, _I, ctypes.c_int64, _I, _P, _I, _P]),
    # maps and in-betweens: the transport read from a time s in both directions
    "foto_maps_from_phi": (_I, [_D, _I, _I, _I, _D, _I, _I, _D]),
    "foto_interp_from_phi": (_I, [_D, _I, _I, _I, _D, _D, _I, _D, _I, _I, _D]),
    "foto_bb_maps": (_I, [_P, _D, _I, _I, _D]),
    "foto_bb_maps_dev": (_I, [_P, _D, _I, _I, _P, _I, _P]),
    "foto_bb_interp_dev": (_I, [_P, ctypes.POINTER(Image), ctypes.POINTER(Image), _I, ctypes.c_int64, ctypes.c_int64,
                                _D, _I, _I, _P, _I, _P]),
    # the transport report: per-plane mass, action, continuity and HJ residual sums
    "foto_bb_report": (_I, [_P, _D]),
    "foto_bb_report_dev": (_I, [_P, _P, _P]),
    "foto_report_from_state": (_I, [_D, _D, _D, _D, _I, _I, _I, _D]),
    "foto_gn_plan_solve_dev": (_I, [_P, ctypes.POINTER(Image), ctypes.POINTER(Image), _P, _I, _I, _P,
                                    ctypes.POINTER(_I)]),
    # coarse-to-fine GN: pyramid, warping, increment solves
    "foto_gn_pyr_sizes": (_I, [_I, _I, _I, _I, ctypes.POINTER(_I), ctypes.POINTER(_I), _I, ctypes.POINTER(_I)]),
    "foto_gn_pyr_opts_default": (_I, [ctypes.POINTER(GNPyrOpts)]),
    "foto_gn_pyr_create": (_I, [_I, _I, _Dbl, _Dbl, ctypes.POINTER(GNPyrOpts), ctypes.POINTER(_P)]),
    "foto_gn_pyr_destroy": (None, [_P]),
    "foto_gn_pyr_device": (_I, [_P]),
    "foto_gn_pyr_solve": (_I, [_P, _D, _D, _D, _D, _D, ctypes.POINTER(GNPyrStats)]),
    "foto_gn_pyr_solve_dev": (_I, [_P, ctypes.POINTER(Image), ctypes.POINTER(Image), _P, _I, _I, _P,
                                   ctypes.POINTER(GNPyrStats)]),
    "foto_pyr_down": (_I, [_D, _D, _I, _I, _D, _D]),
    "foto_pyr_up": (_I, [_D, _D, _D, _I, _I, _I, _I, _D, _D, _D]),
    "foto_gn_warp_prior": (_I, [_D, _D, _D, _D, _I, _I, _D]),
    "foto_gn_solve_prior": (_I, [_D, _D, _I, _I, _Dbl, _Dbl, _Dbl, _I, _D, _D, _D, _D, _D, _D, ctypes.POINTER(_I)]),
    # TV-L1 flow with an illumination channel
    "foto_tvl1_opts_default": (_I, [ctypes.POINTER(TVL1Opts)]),
    "foto_tvl1_create": (_I, [_I, _I, ctypes.POINTER(TVL1Opts), ctypes.POINTER(_P)]),
    "foto_tvl1_destroy": (None, [_P]),
    "foto_tvl1_device": (_I, [_P]),
    "foto_tvl1_solve": (_I, [_P, _D, _D, _D, _D, _D, ctypes.POINTER(TVL1Stats)]),
    "foto_tvl1_solve_dev": (_I, [_P, ctypes.POINTER(Image), ctypes.POINTER(Image), _P, _I, _I, _P,
                                 ctypes.POINTER(TVL1Stats)]),
    "foto_tvl1_coeffs": (_I, [_D, _D, _D, _D, _I, _I, _Dbl, _D]),
    "foto_tvl1_iterate": (_I, [_D, _D, _D, _I, _I, _Dbl, _Dbl, _Dbl, _I, _I]),
    "foto_warp_dev": (_I, [_P, _P, _P, _P, _I, _I, _P, _P]),
    "foto_flow_errors_dev": (_I, [_P, _P, _P, _P, _I, _I, _D, _P]),
    "foto_intensity_error_dev": (_I, [_P, _P, _I, _I, _D, _P]),
    "foto_dev_malloc": (_I, [ctypes.c_size_t, ctypes.POINTER(_P)]),
    "foto_dev_free": (_I, [_P]),
    "foto_dev_memcpy": (_I, [_P, _P, ctypes.c_size_t, _I]),
    # rendering: flow buffers -> images on the device
    "foto_flow_check": (_I, [ctypes.POINTER(Flow), _I, _I]),
    "foto_render_warp_dev": (_I, [ctypes.POINTER(Image), _I, ctypes.c_int64, ctypes.POINTER(Flow), _I, _I, _I, _P, _I,
                                  _P]),
    "foto_render_lum_dev": (_I, [ctypes.POINTER(Flow), _I, _I, _P, _P]),
    "foto_render_color_dev": (_I, [ctypes.POINTER(Flow), _I, _I, _Dbl, _P, _P, _P]),
    # scoring: flow and frame buffers -> statistics tables on the device
    "foto_score_opts_default": (_I, [ctypes.POINTER(ScoreOpts)]),
    "foto_score_check": (_I, [ctypes.POINTER(Flow), ctypes.POINTER(Flow), ctypes.POINTER(Image), _I, _I,
                              ctypes.POINTER(ScoreOpts)]),
    "foto_score_flow_dev": (_I, [ctypes.POINTER(Flow), ctypes.POINTER(Flow), ctypes.POINTER(Image), _I, _I,
                                 ctypes.POINTER(ScoreOpts), _P, _P, _I, _P]),
    "foto_score_flow": (_I, [ctypes.POINTER(Flow), ctypes.POINTER(Flow), ctypes.POINTER(Image), _I, _I,
                             ctypes.POINTER(ScoreOpts), _P, _P, _I]),
    "foto_score_frames_dev": (_I, [ctypes.POINTER(Image), _I, ctypes.c_int64, ctypes.POINTER(Image),
                                   ctypes.POINTER(Image), _I, _I, _Dbl, _P, _P]),
    # flow algebra: compose, invert and cross-check flow buffers on the device
    "foto_chain_check": (_I, [ctypes.POINTER(Flow), ctypes.POINTER(Flow), _I, _I]),
    "foto_flow_compose_dev": (_I, [ctypes.POINTER(Flow), _I, _I, _I, _P, _I, _I, _P]),
    "foto_flow_invert_dev": (_I, [ctypes.POINTER(Flow), _I, _I, _I, _P, _I, _I, _P]),
    "foto_flow_consistency_dev": (_I, [ctypes.POINTER(Flow), ctypes.POINTER(Flow), _I, _I, _Dbl, _Dbl, _P, _P, _I, _P,
                                       _P]),
    # flow filtering: the guided weighted median and hole filling of flow buffers
    "foto_median_opts_default": (_I, [ctypes.POINTER(MedianOpts)]),
    "foto_filter_check": (_I, [ctypes.POINTER(Flow), ctypes.POINTER(Image), _I, ctypes.c_int64, ctypes.POINTER(Image),
                               _I, _I, ctypes.POINTER(MedianOpts)]),
    "foto_flow_median_dev": (_I, [ctypes.POINTER(Flow), ctypes.POINTER(Image), _I, ctypes.c_int64,
                                  ctypes.POINTER(Image), _I, _I, ctypes.POINTER(MedianOpts), _P, _I, _I, _P, _P, _P]),
    # frame preparation: grey, PIL-exact resize, pair normalisation, illumination, difference
    "foto_prep_gray_dev": (_I, [ctypes.POINTER(Image), _I, ctypes.c_int64, _I, _I, _P, _P]),
    "foto_resize_coeffs": (_I, [_I, _I, _I, ctypes.POINTER(_I), ctypes.POINTER(_I), _D, ctypes.POINTER(ctypes.c_int32),
                                _I]),
    "foto_resize_plan_create": (_I, [_I, _I, _I, _I, _I, ctypes.POINTER(_P)]),
    "foto_resize_plan_destroy": (None, [_P]),
    "foto_resize_plan_device": (_I, [_P]),
    "foto_resize_plan_info": (_I, [_P, ctypes.POINTER(_I)]),
    "foto_resize_dev": (_I, [_P, ctypes.POINTER(Image), _I, ctypes.c_int64, _P, _I, _I, _P]),
    "foto_flow_resize_dev": (_I, [_P, ctypes.POINTER(Flow), _P, _I, _P]),
    "foto_prep_normalize_pair_dev": (_I, [ctypes.POINTER(Image), ctypes.POINTER(Image), _I, _I, _P, _P, _I, _D, _P]),
    "foto_prep_illuminate_dev": (_I, [ctypes.POINTER(Image), _I, _I, ctypes.POINTER(LumShape), _I, _P, _I, _P]),
    "foto_prep_diff_dev": (_I, [ctypes.POINTER(Image), ctypes.POINTER(Image), _I, _I, _P, _I, _D, _P]),
    # sparse tracking: Shi-Tomasi corners, pyramidal Lucas-Kanade, a dense flow sampled at points
    "foto_corner_opts_default": (_I, [ctypes.POINTER(CornerOpts)]),
    "foto_corners_dev": (_I, [ctypes.POINTER(Image), _I, _I, ctypes.POINTER(CornerOpts), _I, _P, _I, _P,
                              ctypes.POINTER(_I), _P, _P]),
    "foto_lk_opts_default": (_I, [ctypes.POINTER(LKOpts)]),
    "foto_lk_create": (_I, [_I, _I, ctypes.POINTER(LKOpts), ctypes.POINTER(_P)]),
    "foto_lk_destroy": (None, [_P]),
    "foto_lk_device": (_I, [_P]),
    "foto_lk_set_frames_dev": (_I, [_P, ctypes.POINTER(Image), ctypes.POINTER(Image), _P]),
    "foto_lk_track_dev": (_I, [_P, _P, _I, ctypes.c_int64, _I, _P, _Dbl, _P, _I, _P, _P, _P, _P]),
    "foto_flow_sample_dev": (_I, [ctypes.POINTER(Flow), _I, _I, _P, _I, ctypes.c_int64, _P, _I, _P]),
    # global motion: RANSAC fit of a parametric model, its flow field, the residual flow
    "foto_motion_opts_default": (_I, [ctypes.POINTER(MotionOpts)]),
    "foto_motion_fit_dev": (_I, [_P, _I, _P, _I, _P, ctypes.c_int64, _I, _I, ctypes.POINTER(MotionOpts), _P, _I, _P, _P,
                                 _P, _P, _P]),
    "foto_motion_fit_flow_dev": (_I, [ctypes.POINTER(Flow), _I, _I, _I, _I, _P, ctypes.POINTER(MotionOpts), _P, _I, _P,
                                      _P, _P, _P, _P]),
    "foto_motion_field_dev": (_I, [_P, _I, _I, _I, _P, _I, _I, _P]),
    "foto_motion_residual_dev": (_I, [ctypes.POINTER(Flow), _P, _I, _I, _I, _P, _P]),
    # feature matching: binary descriptors at points, the Hamming matcher, the mutual check
    "foto_describe_opts_default": (_I, [ctypes.POINTER(DescribeOpts)]),
    "foto_match_opts_default": (_I, [ctypes.POINTER(MatchOpts)]),
    "foto_describe_dev": (_I, [ctypes.POINTER(Image), _I, _I, _P, _I, ctypes.c_int64, ctypes.POINTER(DescribeOpts), _P, _P,
                               _P, _P, _P, _P]),
    "foto_match_dev": (_I, [_P, _P, _P, _I, ctypes.c_int64, _P, _P, _P, _I, ctypes.c_int64, ctypes.POINTER(MatchOpts),
                            _P, _P, _P, _P, _I, _P]),
    "foto_match_cross_dev": (_I, [_P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P]),
    # entropic transport: convolutional Sinkhorn, its flow and its cost
    "foto_sinkhorn_opts_default": (_I, [ctypes.POINTER(SinkhornOpts)]),
    "foto_sinkhorn_create": (_I, [_I, _I, ctypes.POINTER(SinkhornOpts), _D, ctypes.POINTER(_P)]),
    "foto_sinkhorn_destroy": (None, [_P]),
    "foto_sinkhorn_set_frames_dev": (_I, [_P, ctypes.POINTER(Image), ctypes.POINTER(Image), _P]),
    "foto_sinkhorn_iterate_dev": (_I, [_P, _I, _P]),
    "foto_sinkhorn_flow_dev": (_I, [_P, _I, _P, _I, _I, _P, _P]),
    "foto_sinkhorn_info_dev": (_I, [_P, _P, _P]),
    "foto_sinkhorn_scalings_dev": (_I, [_P, _P, _P, _P]),
    "foto_sinkhorn_solve": (_I, [_P, _D, _D, _I, _D, _D, _D]),
    "foto_sinkhorn_solve_dev": (_I, [_P, ctypes.POINTER(Image), ctypes.POINTER(Image), _I, _P, _I, _I, _P]),
}

_lib = None


def load(path):
    """A libfoto build at `path` with every signature of include/foto.h set (lib() is the
    product library; tests load libfoto_mockrccl.so, the in-process RCCL transport, this way)."""
    if not os.path.exists(path):
        raise FotoError(f"libfoto.so not found at {path}; build it with "
                        "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C csrc`")
    L = ctypes.CDLL(path)
    lax = os.environ.get("FOTO_LIB_LAX") == "1"   # A/B runs against older builds (tools/ab_lib.sh)
    for name, (res, args) in SIGNATURES.items():
        if lax and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    return L


def lib():
    """Load libfoto.so (once).  Raises if it is missing: there is no CPU fallback."""
    global _lib
    if _lib is None:
        _lib = load(LIB_PATH)
    return _lib


def check(rc, L=None):
    if rc < 0:
        msg = (L or lib()).foto_last_error().decode(errors="replace")
        if rc == FOTO_ERR_BC:
            raise NotImplementedError("These boundary conditions are not implemented")
        raise FotoError(f"libfoto error {rc}: {msg}")
    return rc


def dptr(a):
    return a.ctypes.data_as(_D)


def f64(a, n=None, name="array"):
    """C-contiguous float64 copy-free view (or copy) with an optional length check."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel())
    if n is not None and a.size != n:
        raise ValueError(f"{name}: expected {n} values, got {a.size}")
    return a


def device_count():
    n = ctypes.c_int(0)
    check(lib().foto_device_count(ctypes.byref(n)))
    return n.value
