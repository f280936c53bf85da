"""linesegmentdetector-slam_amd -- MI355X-native LSD line-feature extractor.

Python host-side mirror of the reference interface for the hot path
(``mylsd::myLineSegmentDetector``, LSD/myLSD.h:132) on top of the C ABI of ``liblsdhip.so``
(include/lsd_hip.h).  The directory name contains a hyphen, import it with::

    lsd = importlib.import_module("linesegmentdetector-slam_amd")

There is NO CPU fallback: without the built HIP library, or without a GPU, every entry point
raises.  (The CPU oracle under oracle/ is test infrastructure and is never imported from here.)
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblsdhip.so")

# ---- constants mirrored from include/lsd_hip.h -------------------------------------------------
LSD_OK, LSD_ERR_INVALID, LSD_ERR_NO_DEVICE, LSD_ERR_HIP, LSD_ERR_UNSUPPORTED, LSD_ERR_CAPACITY, LSD_ERR_NOMEM, LSD_ERR_INTERNAL = range(8)
LSD_FLAG_WRITEBACK_MAP = 1
STAGE_ALL, STAGE_GAUSS, STAGE_GRAD, STAGE_SORT, STAGE_REGION = range(5)
(DBG_GAUSS, DBG_MAG, DBG_DEG, DBG_STATE, DBG_ORDER, DBG_ORDER_VAL, DBG_NB, DBG_MAXGRAD, DBG_RECS, DBG_SEEDS,
 DBG_NSEED, DBG_STATS, DBG_SINCOS, DBG_PW, DBG_GRAD_TIES) = range(1, 16)

# LSD defaults, LSD/baseFunc.h:64-68
lsd_sca, lsd_sig, lsd_angThre, lsd_denThre, pseBin = 0.3, 0.6, 22.5, 0.7, 1024
z_occ_max_dis = 1.0   # LSD/baseFunc.h:60
HOST_MAX_LINES_DEFAULT = 8192   # a fresh context's line capacity per image of run / run_batch (lsd_set_host_max_lines in lsd_hip.h)
rdp_leastPoint, rdp_threLine, rdp_leastDist = 3, 0.08, 0.5   # RDP defaults, LSD/baseFunc.h:70-72


class lsd_params(C.Structure):
    _fields_ = [("sca", C.c_double), ("sig", C.c_double), ("angThre", C.c_double), ("denThre", C.c_double),
                ("pseBin", C.c_int)]


class lsd_line(C.Structure):  # == structLinesInfo, LSD/baseFunc.h:33-44
    _fields_ = [(n, C.c_double) for n in ("k", "b", "dx", "dy", "x1", "y1", "x2", "y2", "len")] + [("orient", C.c_int)]


# numpy view of structLinesInfo (80 bytes incl. tail padding)
LINE_DTYPE = np.dtype([("k", "f8"), ("b", "f8"), ("dx", "f8"), ("dy", "f8"), ("x1", "f8"), ("y1", "f8"),
                       ("x2", "f8"), ("y2", "f8"), ("len", "f8"), ("orient", "i4"), ("_pad", "i4")])
SEED_DTYPE = np.dtype([("order_idx", "i4"), ("x", "i4"), ("y", "i4"), ("num", "i4"), ("outcome", "i4"),
                       ("final_num", "i4"), ("logNFA", "f8")])
assert LINE_DTYPE.itemsize == 80 == C.sizeof(lsd_line)


class lsd_map_param(C.Structure):      # structMapParam, LSD/baseFunc.h:25-31
    _fields_ = [("oriMapCol", C.c_int), ("oriMapRow", C.c_int), ("mapResol", C.c_double), ("mapOriX", C.c_double), ("mapOriY", C.c_double)]


LSD_MAX_MAPS = 64
LSD_SCAN_MAX_LEN = 4096                                               # lsd_set_scan_capacity's upper limit (readings per scan)


class lsd_map_ref(C.Structure):        # one device-resident map of the fleet entries (include/lsd_hip.h)
    _fields_ = [("d_map_cache", C.c_void_p), ("d_map_lines", C.c_void_p), ("d_n_map", C.c_void_p), ("cols", C.c_int), ("rows", C.c_int),
                ("n_map", C.c_int), ("mapResol", C.c_double), ("mapOriX", C.c_double), ("mapOriY", C.c_double)]


# numpy view of lsd_map_ref: a table is an array of these (the pointers as integers, 0 = NULL)
MAP_REF_DTYPE = np.dtype([("d_map_cache", "u8"), ("d_map_lines", "u8"), ("d_n_map", "u8"), ("cols", "i4"), ("rows", "i4"), ("n_map", "i4"),
                          ("_pad", "i4"), ("mapResol", "f8"), ("mapOriX", "f8"), ("mapOriY", "f8")])
assert MAP_REF_DTYPE.itemsize == 64 == C.sizeof(lsd_map_ref)


class lsd_map_frame(C.Structure):      # what turns metres into a map's pixels: the frame a carry's state is in (include/lsd_hip.h)
    _fields_ = [("mapResol", C.c_double), ("mapOriX", C.c_double), ("mapOriY", C.c_double)]


class lsd_position(C.Structure):  # == structPosition, LSD/baseFunc.h:46-50
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("ang", C.c_double)]


POS_DTYPE = np.dtype([("x", "f8"), ("y", "f8"), ("ang", "f8")])


# correlative scan-to-grid matching (include/lsd_hip.h): the smear table, the search window and the record of one matched scan
class lsd_grid_smear(C.Structure):     # radius 0..7, w[|dv|][|du|]
    _fields_ = [("radius", C.c_int), ("w", (C.c_uint8 * 8) * 8)]


class lsd_grid_search(C.Structure):
    _fields_ = [("wx", C.c_int), ("wy", C.c_int), ("na", C.c_int), ("ang_step", C.c_double), ("min_beams", C.c_uint32),
                ("min_num", C.c_uint32), ("min_den", C.c_uint32)]


class lsd_grid_match(C.Structure):     # the C side's lsd_grid_match_rec (struct lsd_grid_match)
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("ang", C.c_double), ("score", C.c_uint32), ("n_beams", C.c_uint32), ("di", C.c_int32),
                ("dj", C.c_int32), ("da", C.c_int32), ("flags", C.c_uint32), ("score_prior", C.c_uint32), ("reserved", C.c_uint32)]


GRID_MATCH_DTYPE = np.dtype([("x", "f8"), ("y", "f8"), ("ang", "f8"), ("score", "u4"), ("n_beams", "u4"), ("di", "i4"), ("dj", "i4"),
                             ("da", "i4"), ("flags", "u4"), ("score_prior", "u4"), ("reserved", "u4")])
assert GRID_MATCH_DTYPE.itemsize == 56 == C.sizeof(lsd_grid_match) and C.sizeof(lsd_grid_smear) == 68 and C.sizeof(lsd_grid_search) == 40
GRID_MATCH_ACCEPTED, GRID_MATCH_SKIPPED = 1, 2
GRID_MATCH_MR_STATS_DTYPE = np.dtype([("blocks", "u4"), ("refined", "u4"), ("fine", "u4"), ("lower_bound", "u4")])   # lsd_grid_match_mr_stats
assert GRID_MATCH_MR_STATS_DTYPE.itemsize == 16


# the response around a match (include/lsd_hip.h): its parameters (the C side's lsd_grid_response_par) and its record
class lsd_grid_response(C.Structure):
    _fields_ = [("rx", C.c_int), ("ry", C.c_int), ("ra", C.c_int), ("keep_num", C.c_uint32), ("keep_den", C.c_uint32)]


class lsd_grid_response_rec(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("ang", C.c_double), ("cov", C.c_double * 6), ("sub", C.c_double * 3),
                ("m", C.c_int64 * 10), ("score_centre", C.c_uint32), ("n_used", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


GRID_RESPONSE_DTYPE = np.dtype([("x", "f8"), ("y", "f8"), ("ang", "f8"), ("cov", "f8", (6,)), ("sub", "f8", (3,)), ("m", "i8", (10,)),
                                ("score_centre", "u4"), ("n_used", "u4"), ("flags", "u4"), ("reserved", "u4")])
assert GRID_RESPONSE_DTYPE.itemsize == 192 == C.sizeof(lsd_grid_response_rec) and C.sizeof(lsd_grid_response) == 20
(GRID_RESPONSE_VALID, GRID_RESPONSE_NONE, GRID_RESPONSE_X_NOT_PEAK, GRID_RESPONSE_Y_NOT_PEAK, GRID_RESPONSE_A_NOT_PEAK, GRID_RESPONSE_EMPTY,
 GRID_RESPONSE_MISMATCH) = 1, 2, 4, 8, 16, 32, 64
SCORE_DTYPE = np.dtype([("x", "f8"), ("y", "f8"), ("ang", "f8"), ("score", "f8")])   # lsd_match_score


# ray casting on the grid (include/lsd_hip.h): its parameters, the record of a beam and the summary of a scan
class lsd_grid_ray_par(C.Structure):
    _fields_ = [("tol", C.c_double), ("drop_mask", C.c_uint32), ("min_beams", C.c_uint32), ("ok_num", C.c_uint32), ("ok_den", C.c_uint32),
                ("gate", C.c_int)]


GRID_RAY_DTYPE = np.dtype([("r_exp", "f8"), ("r_unk", "f8"), ("cx", "i4"), ("cy", "i4"), ("k_hit", "i4"), ("cls", "u4")])      # lsd_grid_ray
GRID_RAY_SUM_DTYPE = np.dtype([("x", "f8"), ("y", "f8"), ("ang", "f8"), ("n", "u4", (7,)), ("judged", "u4"), ("flags", "u4"),
                               ("pad", "u4")])                                                                                # lsd_grid_ray_sum
assert GRID_RAY_DTYPE.itemsize == 32 and GRID_RAY_SUM_DTYPE.itemsize == 64 and C.sizeof(lsd_grid_ray_par) == 32
(GRID_RAY_NOT_CAST, GRID_RAY_NO_MEASUREMENT, GRID_RAY_AGREE_FREE, GRID_RAY_AGREE, GRID_RAY_SHORT, GRID_RAY_LONG,
 GRID_RAY_UNEXPLORED) = range(7)
GRID_RAY_CLASSES = ("not_cast", "no_measurement", "agree_free", "agree", "short", "long", "unexplored")
GRID_RAY_CONSISTENT, GRID_RAY_SKIPPED = 1, 2

# global scan-to-grid localisation (include/lsd_hip.h): its parameters, the record of a scan and its statistics
class lsd_grid_locate_par(C.Structure):
    _fields_ = [("x0", C.c_int), ("y0", C.c_int), ("nx", C.c_int), ("ny", C.c_int), ("ang0", C.c_double), ("ang_step", C.c_double),
                ("n_ang", C.c_int), ("levels", C.c_int), ("max_nodes", C.c_uint32), ("score_floor", C.c_uint32), ("min_beams", C.c_uint32),
                ("min_num", C.c_uint32), ("min_den", C.c_uint32)]


GRID_LOCATE_DTYPE = np.dtype([("x", "f8"), ("y", "f8"), ("ang", "f8"), ("score", "u4"), ("n_beams", "u4"), ("cx", "i4"), ("cy", "i4"),
                              ("a", "i4"), ("flags", "u4"), ("n_best", "u4"), ("lower_bound", "u4"), ("reserved", "u4", (2,))])    # lsd_grid_locate_rec
GRID_LOCATE_STATS_DTYPE = np.dtype([("top_nodes", "u4"), ("frontier", "u4", (9,)), ("scored", "u4"), ("reserved", "u4")])          # lsd_grid_locate_stats
assert GRID_LOCATE_DTYPE.itemsize == 64 == C.sizeof(lsd_grid_locate_par) and GRID_LOCATE_STATS_DTYPE.itemsize == 48
GRID_LOCATE_ACCEPTED, GRID_LOCATE_REJECTED, GRID_LOCATE_NOT_FOUND, GRID_LOCATE_OVERFLOW, GRID_LOCATE_EMPTY = 1, 2, 4, 8, 16
GRID_LOCATE_MAX_LEVELS = 8
GRID_LOCATE_TIGHT_STATS_DTYPE = np.dtype([("top_nodes", "u4"), ("frontier", "u4", (9,)), ("scored", "u4"), ("retried", "u4"), ("bound", "u4", (9,)),
                                          ("first_count", "u4", (9,)), ("reserved", "u4", (2,))])                                      # lsd_grid_locate_tight_stats
assert GRID_LOCATE_TIGHT_STATS_DTYPE.itemsize == 128
GRID_LOCATE_TIGHT_PROBE, GRID_LOCATE_TIGHT_RETRY = 1, 2

# FeatureAssociation (include/lsd_hip.h): the 9-state filter (P column-major, as Eigen stores kalman_P) and the per-frame report
FA_STATE_DTYPE = np.dtype([("x", "f8", (9,)), ("P", "f8", (81,))])
FA_REPORT_DTYPE = np.dtype([("estimate", POS_DTYPE), ("score", "f8"), ("scan_pose", POS_DTYPE), ("n_pairs", "i4"), ("n_kept", "i4"),
                            ("branch", "i4"), ("llt", "i4")])
assert FA_STATE_DTYPE.itemsize == 720 and FA_REPORT_DTYPE.itemsize == 72
FA_RESET, FA_FIRST, FA_UKF = range(3)
# lsd_fa_carry: the replay loop's variables between calls of lsd_enqueue_localize_resume_device (plain bytes: copy, keep, save, restore)
FA_CARRY_DTYPE = np.dtype([("state", FA_STATE_DTYPE), ("odom", POS_DTYPE), ("ang_sum", "f8"), ("ang_count", "f8"), ("frames", "i4"),
                           ("is_offset", "i4")])
assert FA_CARRY_DTYPE.itemsize == 768


# the grid match response fused into a carry (include/lsd_hip.h): its parameters and its report
class lsd_fa_correct(C.Structure):     # the C side's lsd_fa_correct_par
    _fields_ = [("cov_scale", C.c_double), ("floor_xy", C.c_double), ("floor_ang", C.c_double), ("gate", C.c_double)]


FA_CORRECT_DTYPE = np.dtype([("innov", "f8", (3,)), ("d2", "f8"), ("det", "f8"), ("slot", "i4"), ("flags", "u4")])   # lsd_fa_correct_rep
assert FA_CORRECT_DTYPE.itemsize == 48 and C.sizeof(lsd_fa_correct) == 32
(FA_CORRECT_APPLIED, FA_CORRECT_NO_POSE, FA_CORRECT_NOT_FINITE, FA_CORRECT_STALE, FA_CORRECT_NO_RESPONSE, FA_CORRECT_SINGULAR,
 FA_CORRECT_GATED) = 1, 2, 4, 8, 16, 32, 64


# relocalisation on the device (include/lsd_hip.h): the seed's parameters and its report
class lsd_fa_seed(C.Structure):        # the C side's lsd_fa_seed_par
    _fields_ = [("var_xy", C.c_double), ("var_ang", C.c_double), ("cov_scale", C.c_double), ("floor_xy", C.c_double), ("floor_ang", C.c_double),
                ("max_best", C.c_uint32), ("reserved", C.c_uint32)]


FA_SEED_DTYPE = np.dtype([("pose", "f8", (3,)), ("ang_diff", "f8"), ("seq", "i4"), ("slot", "i4"), ("flags", "u4"), ("loc_flags", "u4")])   # lsd_fa_seed_rep
assert FA_SEED_DTYPE.itemsize == 48 and C.sizeof(lsd_fa_seed) == 48
(FA_SEED_SEEDED, FA_SEED_UNUSED, FA_SEED_BAD_PICK, FA_SEED_HAS_POSE, FA_SEED_NOT_LOCATED, FA_SEED_AMBIGUOUS, FA_SEED_NO_RESPONSE,
 FA_SEED_NOT_FINITE) = 1, 2, 4, 8, 16, 32, 64, 128


# the pose graph (include/lsd_hip.h, "pose graph"): its records, parameters and reports
class lsd_pg_append(C.Structure):      # the C side's lsd_pg_append_par
    _fields_ = [("min_dist", C.c_double), ("min_ang", C.c_double), ("info", C.c_double * 6)]


class lsd_pg_closure(C.Structure):     # the C side's lsd_pg_closure_par
    _fields_ = [("cov_scale", C.c_double), ("floor_xy", C.c_double), ("floor_ang", C.c_double)]


class lsd_pg_relax(C.Structure):       # the C side's lsd_pg_relax_par
    _fields_ = [("lambda0", C.c_double), ("lambda_min", C.c_double), ("up", C.c_double), ("down", C.c_double), ("cg_tol", C.c_double),
                ("eps", C.c_double), ("iters", C.c_int32), ("cg_iters", C.c_int32)]


class lsd_pg_robust(C.Structure):      # the C side's lsd_pg_robust_par
    _fields_ = [("kernel", C.c_int32), ("scope", C.c_uint32), ("delta", C.c_double)]


class lsd_pg_prune(C.Structure):       # the C side's lsd_pg_prune_par
    _fields_ = [("gate", C.c_double), ("max_reject", C.c_int32), ("reserved", C.c_int32)]


class lsd_pg_precond(C.Structure):     # the C side's lsd_pg_precond_par
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32)]


PG_HEAD_DTYPE = np.dtype([("n_nodes", "i4"), ("n_edges", "i4")])
PG_NODE_DTYPE = np.dtype([("x", "f8"), ("y", "f8"), ("ang", "f8"), ("raw", "f8", (3,)), ("flags", "u4"), ("track", "i4"), ("reserved", "u8")])
PG_EDGE_DTYPE = np.dtype([("i", "i4"), ("j", "i4"), ("flags", "u4"), ("reserved", "u4"), ("z", "f8", (3,)), ("info", "f8", (6,)), ("chi2", "f8")])
PG_TRACK_DTYPE = np.dtype([("last", "i4"), ("reserved", "i4"), ("raw", "f8", (3,))])
PG_APPEND_REP_DTYPE = np.dtype([("nodes", "i4"), ("edges", "i4"), ("dropped", "i4"), ("flags", "u4")])
PG_NEAR_DTYPE = np.dtype([("anchor", "i4"), ("query", "i4"), ("n_cand", "i4"), ("reserved", "i4"), ("d2", "f8")])
PG_CLOSURE_REP_DTYPE = np.dtype([("edge", "i4"), ("flags", "u4"), ("det", "f8")])
PG_RELAX_REP_DTYPE = np.dtype([("chi2_before", "f8"), ("chi2_after", "f8"), ("lambda", "f8"), ("iters", "i4"), ("cg_iters", "i4"), ("accepted", "i4"),
                               ("rejected", "i4"), ("skipped_edges", "i4"), ("singular_nodes", "i4"), ("flags", "u4"), ("reserved", "u4")])
assert (PG_HEAD_DTYPE.itemsize, PG_NODE_DTYPE.itemsize, PG_EDGE_DTYPE.itemsize, PG_TRACK_DTYPE.itemsize) == (8, 64, 96, 32)
assert (PG_APPEND_REP_DTYPE.itemsize, PG_NEAR_DTYPE.itemsize, PG_CLOSURE_REP_DTYPE.itemsize, PG_RELAX_REP_DTYPE.itemsize) == (16, 24, 16, 56)
assert (C.sizeof(lsd_pg_append), C.sizeof(lsd_pg_closure), C.sizeof(lsd_pg_relax)) == (64, 24, 56)
PG_NODE_FIXED = 1
PG_EDGE_DISABLED, PG_EDGE_CLOSURE = 1, 2
PG_APPEND_NODES_FULL, PG_APPEND_EDGES_FULL = 1, 2
PG_CLOSURE_APPENDED, PG_CLOSURE_NO_ANCHOR, PG_CLOSURE_NO_RESPONSE, PG_CLOSURE_NOT_FINITE, PG_CLOSURE_SINGULAR, PG_CLOSURE_FULL = 1, 2, 4, 8, 16, 32
PG_RELAX_CONVERGED, PG_RELAX_BREAKDOWN, PG_RELAX_NOT_FINITE = 1, 2, 4
PG_MAX_NODES, PG_MAX_EDGES = 16384, 65536
# the robust relaxation and the rejection of closures
PG_ROBUST_REP_DTYPE = np.dtype([("chi2_plain", "f8"), ("w_min", "f8"), ("downweighted", "i4"), ("w_min_edge", "i4")])
PG_PRUNE_REP_DTYPE = np.dtype([("candidates", "i4"), ("rejected", "i4"), ("worst_edge", "i4"), ("closures_left", "i4"), ("worst_chi2", "f8")])
assert (PG_ROBUST_REP_DTYPE.itemsize, PG_PRUNE_REP_DTYPE.itemsize, C.sizeof(lsd_pg_robust), C.sizeof(lsd_pg_prune)) == (24, 24, 16, 16)
PG_EDGE_REJECTED = 4
PG_KERNEL_NONE, PG_KERNEL_HUBER, PG_KERNEL_GM = 0, 1, 2
PG_ROBUST_CLOSURES, PG_ROBUST_ALL = 0, 1
PG_MAX_REJECT = 64
# the relaxation's preconditioner
PG_PRECOND_REP_DTYPE = np.dtype([("chain_edges", "i4"), ("paths", "i4"), ("longest_path", "i4"), ("fallbacks", "i4")])
assert (PG_PRECOND_REP_DTYPE.itemsize, C.sizeof(lsd_pg_precond)) == (16, 8)
PG_PRECOND_BLOCK, PG_PRECOND_CHAIN = 0, 1
# marginal covariances and the gate on new closures


class lsd_pg_marg(C.Structure):        # the C side's lsd_pg_marg_par
    _fields_ = [("cg_tol", C.c_double), ("cg_iters", C.c_int32), ("precond", C.c_int32), ("slots", C.c_int32), ("reserved", C.c_int32)]


PG_MARG_QUERY_DTYPE = np.dtype([("kind", "i4"), ("a", "i4"), ("b", "i4"), ("reserved", "i4")])
PG_MARG_REC_DTYPE = np.dtype([("cov", "f8", (9,)), ("steps", "i4", (3,)), ("flags", "u4"), ("kind", "i4"), ("edge", "i4"), ("i", "i4"), ("j", "i4")])
PG_MARG_REP_DTYPE = np.dtype([("n_nodes", "i4"), ("n_edges", "i4"), ("skipped_edges", "i4"), ("singular_nodes", "i4"), ("chain_edges", "i4"),
                              ("paths", "i4"), ("longest_path", "i4"), ("fallbacks", "i4")])
PG_VET_REP_DTYPE = np.dtype([("d2", "f8"), ("det", "f8"), ("edge", "i4"), ("flags", "u4")])
assert (PG_MARG_QUERY_DTYPE.itemsize, PG_MARG_REC_DTYPE.itemsize, PG_MARG_REP_DTYPE.itemsize, PG_VET_REP_DTYPE.itemsize,
        C.sizeof(lsd_pg_marg)) == (16, 104, 32, 24, 24)
PG_MARG_NODE, PG_MARG_PAIR, PG_MARG_NEW_EDGE = 0, 1, 2
PG_MARG_CONVERGED_0, PG_MARG_MAXED_0, PG_MARG_BREAKDOWN_0, PG_MARG_CONVERGED = 0x1, 0x10, 0x100, 0x7
PG_MARG_FIXED, PG_MARG_SINGULAR, PG_MARG_BAD_QUERY, PG_MARG_NO_EDGE = 0x1000, 0x2000, 0x4000, 0x8000
PG_VET_UNUSED, PG_VET_NO_EDGE, PG_VET_SKIPPED, PG_VET_NO_MARGINAL, PG_VET_SINGULAR, PG_VET_REJECTED, PG_VET_PASSED = 1, 2, 4, 8, 16, 32, 64
PG_MARG_MAX_QUERIES, PG_MARG_MAX_SLOTS = 65536, 1024
# place recognition


class lsd_pg_place(C.Structure):       # the C side's lsd_pg_place_par
    _fields_ = [("gap", C.c_int32), ("window", C.c_int32), ("spread", C.c_int32), ("k", C.c_int32), ("pick", C.c_int32), ("max_dist", C.c_uint32),
                ("min_sectors", C.c_uint32), ("reserved", C.c_uint32)]


PG_DESC_SECTORS, PG_PLACE_MAX = 64, 8
PG_DESC_DTYPE = np.dtype([("v", "u1", (PG_DESC_SECTORS,)), ("n_hits", "u4"), ("n_sectors", "u2"), ("valid", "u2")])
PG_PLACE_REC_DTYPE = np.dtype([("anchor", "i4"), ("shift", "i4"), ("dist", "u4"), ("reserved", "u4")])
PG_PLACE_REP_DTYPE = np.dtype([("query", "i4"), ("n_cand", "i4"), ("n_picked", "i4"), ("reserved", "i4")])
assert (PG_DESC_DTYPE.itemsize, PG_PLACE_REC_DTYPE.itemsize, PG_PLACE_REP_DTYPE.itemsize, C.sizeof(lsd_pg_place)) == (72, 16, 16, 32)
# every loop of a track in one pass


class lsd_pg_loops(C.Structure):       # the C side's lsd_pg_loops_par
    _fields_ = [("max_loops", C.c_int32), ("spread", C.c_int32)]


PG_LOOPS_MAX = 64
PG_LOOP_REC_DTYPE = np.dtype([("query", "i4"), ("anchor", "i4"), ("shift", "i4"), ("dist", "u4")])
PG_LOOPS_REP_DTYPE = np.dtype([("n_pairs", "i4"), ("n_known", "i4"), ("n_loops", "i4"), ("reserved", "i4")])
assert (PG_LOOP_REC_DTYPE.itemsize, PG_LOOPS_REP_DTYPE.itemsize, C.sizeof(lsd_pg_loops)) == (16, 16, 8)
# redundant keyframes retired, the store compacted


class lsd_pg_reduce(C.Structure):      # the C side's lsd_pg_reduce_par
    _fields_ = [("cell", C.c_double), ("ang_bin", C.c_double), ("keep", C.c_int32), ("max_run", C.c_int32)]


PG_REDUCE_REP_DTYPE = np.dtype([("nodes_before", "i4"), ("edges_before", "i4"), ("nodes_after", "i4"), ("edges_after", "i4"), ("redundant", "i4"),
                                ("marked", "i4"), ("retired", "i4"), ("runs", "i4"), ("runs_kept", "i4"), ("longest_run", "i4"),
                                ("dropped_edges", "i4"), ("flags", "u4")])
assert (PG_REDUCE_REP_DTYPE.itemsize, C.sizeof(lsd_pg_reduce)) == (48, 24)
PG_EDGE_CONTRACTED = 8
PG_REDUCE_RETIRED, PG_REDUCE_SPLIT = 1, 2


# lsd_comm (include/lsd_hip.h): rank, world, an all-gather callback of device buffers on a stream, and its user pointer
ALL_GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)


class lsd_comm(C.Structure):
    _fields_ = [("rank", C.c_int), ("world", C.c_int), ("all_gather", ALL_GATHER_FN), ("user", C.c_void_p)]


class LsdError(RuntimeError):
    """A non-zero status of the C ABI.  `partial`: where the C side says its outputs are valid nevertheless (LSD_ERR_CAPACITY /
    LSD_ERR_INTERNAL of the gather, LSD_ERR_CAPACITY of FeatureScan), what the call would have returned."""
    def __init__(self, status, msg, partial=None):
        super().__init__("lsd_hip status %d: %s" % (status, msg))
        self.status = status
        self.partial = partial


# ---- the C ABI (include/lsd_hip.h), listed once: name -> (restype, argtypes) --------------------------------------------------
_vp, _i, _sz, _dbl = C.c_void_p, C.c_int, C.c_size_t, C.c_double
_pi, _ppar = C.POINTER(C.c_int), C.POINTER(lsd_params)
_localize_args = [_vp, _vp, _i, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _dbl, _vp, _vp, _vp, _vp]
_maps_args = [_vp, _vp, _i, _vp] + _localize_args[6:16] + _localize_args[17:]   # the map and map_resol -> maps, n_maps, d_map_of
_live_map_args = _localize_args[:6] + [_vp] + _localize_args[6:]      # int n_map -> int map_lines_cap, const int32_t *d_n_map
_ABI = {
    "lsd_create": (_i, [C.POINTER(_vp), _i]),
    "lsd_destroy": (None, [_vp]),
    "lsd_strerror": (C.c_char_p, [_i]),
    "lsd_last_error": (C.c_char_p, [_vp]),
    "lsd_default_params": (None, [_ppar]),
    "lsd_abi_version": (_i, []),
    "lsd_free": (None, [_vp]),
    "lsd_run": (_i, [_vp, _vp, _i, _i, _sz, _ppar, _vp, _sz, C.POINTER(_vp), _pi]),
    "lsd_run_batch": (_i, [_vp, _vp, _i, _i, _i, _ppar, _vp, C.POINTER(_vp), _pi]),
    "lsd_enqueue_batch_device": (_i, [_vp, _vp, _i, _i, _i, _ppar, C.c_uint, _vp, _vp, _i, _vp, _vp]),
    "lsd_reserve": (_i, [_vp, _i, _i, _i]),
    "lsd_synchronize": (_i, [_vp]),
    "lsd_scaled_size": (None, [_i, _i, _dbl, _pi, _pi]),
    "lsd_set_stop_after": (_i, [_vp, _i]),
    "lsd_set_trace": (_i, [_vp, _i]),
    "lsd_set_fused_front": (_i, [_vp, _i]),
    "lsd_set_fused_lines": (_i, [_vp, _i]),
    "lsd_set_region_waves": (_i, [_vp, _i]),
    "lsd_set_region_help": (_i, [_vp, _i]),
    "lsd_debug_set_stamp_budget": (_i, [_vp, C.c_uint]),
    "lsd_debug_poison_front": (_i, [_vp]),
    "lsd_set_cost_history": (_i, [_vp, _i]),
    "lsd_debug_set_tuning": (_i, [_vp, C.c_char_p, _i]),
    "lsd_set_host_max_lines": (_i, [_vp, _i]),
    "lsd_debug_fetch": (_i, [_vp, _i, _i, _vp, _sz]),
    "lsd_last_timings": (_i, [_vp, C.POINTER(C.c_float)]),
    "lsd_map_cache": (_i, [_vp, _vp, _i, _i, _sz, _dbl, _dbl, _vp]),
    "lsd_enqueue_map_cache_device": (_i, [_vp, _vp, _i, _i, _i, _dbl, _dbl, _vp, _vp]),
    "lsd_occupancy_to_map": (_i, [_vp, _vp, _i, _i, _vp, _sz]),
    "lsd_enqueue_occupancy_to_map_device": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "lsd_scan_to_map_match": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _i, _vp, _i, lsd_position, lsd_position, _vp, _i, _dbl, _dbl, _vp]),
    "lsd_enqueue_scan_to_map_match_device": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _i, lsd_position, lsd_position, _vp, _i, _dbl, _dbl, _vp, _vp]),
    "lsd_feature_scan_batch": (_i, [_vp, _vp, _vp, _i, _i, lsd_map_param, _i, _dbl, _dbl, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "lsd_enqueue_feature_scan_batch_device": (_i, [_vp, _vp, _vp, _i, _i, lsd_map_param, _i, _dbl, _dbl, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "lsd_set_scan_capacity": (_i, [_vp, _i]),
    "lsd_scan_capacity": (_i, [_vp]),
    "lsd_shard_range": (None, [_i, _i, _i, _pi, _pi]),
    "lsd_gather_layout": (_i, [_i, _i, _pi, C.POINTER(_sz)]),
    "lsd_comm_from_rccl": (_i, [_vp, C.POINTER(lsd_comm)]),
    "lsd_gather_lines": (_i, [_vp, C.POINTER(lsd_comm), _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "lsd_gather_unpack": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _sz]),
    "lsd_shard_balanced": (_i, [_vp, _i, _i, _vp]),
    "lsd_last_region_cycles": (_i, [_vp, _i, _vp]),
    "lsd_last_sensitivity": (_i, [_vp, _i, _vp]),
    "lsd_fa_initial_state": (None, [_vp]),
    "lsd_feature_association": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _i, _vp, _i, lsd_position, lsd_position, lsd_position, _vp, _vp, _vp]),
    "lsd_enqueue_localize_device": (_i, _localize_args),
    "lsd_localize": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp, _i, _i, _vp, lsd_map_param, _vp, _vp, _vp]),
    "lsd_debug_fa_fuse": (_i, [_vp, _vp, _i, lsd_position, lsd_position, _vp, _vp, _vp]),
    "lsd_fa_carry_init": (None, [_vp, _vp, lsd_position]),
    "lsd_enqueue_localize_resume_device": (_i, _localize_args),
    "lsd_enqueue_localize_live_map_device": (_i, _live_map_args),
    "lsd_enqueue_localize_resume_live_map_device": (_i, _live_map_args),
    "lsd_enqueue_feature_scan_maps_device": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _vp, _i, _i, _dbl, _dbl, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "lsd_enqueue_localize_maps_device": (_i, _maps_args),
    "lsd_enqueue_localize_resume_maps_device": (_i, _maps_args),
    "lsd_enqueue_fa_carry_rebase_device": (_i, [_vp, _vp, _i, _vp, C.c_int32, lsd_map_frame, lsd_map_frame, _vp]),
    "lsd_enqueue_fa_carry_correct_device": (_i, [_vp, _vp, _i, _i, _vp, _sz, _vp, _vp, C.c_int32, lsd_fa_correct, _vp, _vp]),
    "lsd_fa_carry_correct": (_i, [_vp, _vp, _i, _i, _vp, _vp, lsd_fa_correct, _vp]),
    "lsd_enqueue_fa_lost_gather_device": (_i, [_vp, _vp, _i, _i, _vp, _sz, _vp, _vp, _i, _vp, C.c_int32, _i, _vp, _vp, _vp, _vp, _vp]),
    "lsd_fa_lost_gather": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "lsd_enqueue_fa_carry_seed_device": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp, lsd_fa_seed, _vp, _vp]),
    "lsd_fa_carry_seed": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp, lsd_fa_seed, _vp]),
    "lsd_enqueue_map_update_device": (_i, [_vp, _vp, _i, _i, _dbl, _dbl, _ppar, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "lsd_reserve_map_update": (_i, [_vp, _i, _i]),
    "lsd_enqueue_scan_ingest_device": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp]),
    "lsd_enqueue_laserscan_ingest_device": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp]),
    "lsd_enqueue_grid_integrate_device": (_i, [_vp, _vp, _vp, _i, _i, _vp, _sz, lsd_map_param, _dbl, _vp, _vp, _vp]),
    "lsd_enqueue_grid_publish_device": (_i, [_vp, _vp, _vp, _sz, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp]),
    "lsd_grid_integrate": (_i, [_vp, _vp, _vp, _i, _i, _vp, lsd_map_param, _dbl, _vp, _vp]),
    "lsd_enqueue_grid_likelihood_device": (_i, [_vp, _vp, _vp, _i, _i, C.c_uint32, C.c_uint32, C.c_uint32, lsd_grid_smear, _vp, _vp]),
    "lsd_grid_smear_default": (_i, [_dbl, _i, C.POINTER(lsd_grid_smear)]),
    "lsd_enqueue_grid_match_device": (_i, [_vp, _vp, _vp, _i, _i, _vp, _sz, lsd_map_param, _dbl, _vp, lsd_grid_search, _vp, _vp]),
    "lsd_grid_match": (_i, [_vp, _vp, _vp, _i, _i, _vp, lsd_map_param, _dbl, _vp, lsd_grid_search, _vp]),
    "lsd_grid_coarse_bytes": (_sz, [_i, _i, _i]),
    "lsd_enqueue_grid_coarse_device": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "lsd_enqueue_grid_match_mr_device": (_i, [_vp, _vp, _vp, _i, _i, _vp, _sz, lsd_map_param, _dbl, _vp, _vp, _i, lsd_grid_search, _vp, _vp, _vp]),
    "lsd_grid_match_mr": (_i, [_vp, _vp, _vp, _i, _i, _vp, lsd_map_param, _dbl, _vp, _i, lsd_grid_search, _vp, _vp]),
    "lsd_grid_response_volume_bytes": (_sz, [_i, lsd_grid_response]),
    "lsd_enqueue_grid_response_device": (_i, [_vp, _vp, _vp, _i, _i, _vp, _sz, _vp, lsd_map_param, _dbl, _vp, _dbl, lsd_grid_response, _vp, _vp,
                                              _vp]),
    "lsd_grid_response": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, lsd_map_param, _dbl, _vp, _dbl, lsd_grid_response, _vp, _vp]),
    "lsd_enqueue_grid_raycast_device": (_i, [_vp, _vp, _vp, _i, _i, _vp, _sz, lsd_map_param, _dbl, _vp, lsd_grid_ray_par, _vp, _vp, _vp, _vp]),
    "lsd_grid_raycast": (_i, [_vp, _vp, _vp, _i, _i, _vp, lsd_map_param, _dbl, _vp, lsd_grid_ray_par, _vp, _vp, _vp]),
    "lsd_grid_pyramid_bytes": (_sz, [_i, _i, _i]),
    "lsd_grid_pyramid_offset": (_sz, [_i, _i, _i]),
    "lsd_enqueue_grid_pyramid_device": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "lsd_grid_locate_workspace_bytes": (_sz, [_i, _i, lsd_grid_locate_par]),
    "lsd_enqueue_grid_locate_device": (_i, [_vp, _vp, _vp, _i, _i, lsd_map_param, _dbl, _vp, lsd_grid_locate_par, _vp, _vp, _vp]),
    "lsd_grid_locate": (_i, [_vp, _vp, _vp, _i, _i, lsd_map_param, _dbl, _vp, lsd_grid_locate_par, _vp, _vp]),
    "lsd_grid_locate_tight_workspace_bytes": (_sz, [_i, _i, lsd_grid_locate_par]),
    "lsd_enqueue_grid_locate_tight_device": (_i, [_vp, _vp, _vp, _i, _i, lsd_map_param, _dbl, _vp, lsd_grid_locate_par, C.c_uint32, _vp, _vp, _vp]),
    "lsd_grid_locate_tight": (_i, [_vp, _vp, _vp, _i, _i, lsd_map_param, _dbl, _vp, lsd_grid_locate_par, C.c_uint32, _vp, _vp]),
    "lsd_enqueue_pg_append_device": (_i, [_vp, _vp, _vp, _i, _i, _vp, _sz, _vp, _vp, _i, _vp, _i, _vp, C.c_int32, _vp, _vp, _i, lsd_pg_append, _vp, _vp]),
    "lsd_enqueue_pg_near_device": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _dbl, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lsd_enqueue_pg_closure_device": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp, lsd_pg_closure, _vp, _vp]),
    "lsd_pg_workspace_bytes": (_sz, [_i, _i]),
    "lsd_enqueue_pg_relax_device": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, lsd_pg_relax, _vp, _vp, _vp]),
    "lsd_pg_relax": (_i, [_vp, _vp, _i, _vp, _i, lsd_pg_relax, _vp]),
    "lsd_enqueue_pg_relax_robust_device": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, lsd_pg_relax, lsd_pg_robust, _vp, _vp, _vp, _vp]),
    "lsd_enqueue_pg_prune_device": (_i, [_vp, _i, _vp, _vp, _i, lsd_pg_prune, _vp, _vp]),
    "lsd_pg_relax_robust": (_i, [_vp, _vp, _i, _vp, _i, lsd_pg_relax, lsd_pg_robust, _vp, _vp]),
    "lsd_pg_workspace_pc_bytes": (_sz, [_i, _i, _i]),
    "lsd_enqueue_pg_relax_pc_device": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, lsd_pg_relax, lsd_pg_robust, lsd_pg_precond, _vp, _vp, _vp, _vp, _vp]),
    "lsd_pg_relax_pc": (_i, [_vp, _vp, _i, _vp, _i, lsd_pg_relax, lsd_pg_robust, lsd_pg_precond, _vp, _vp, _vp]),
    "lsd_pg_marginals_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "lsd_enqueue_pg_marginals_device": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, lsd_pg_marg, _vp, _vp, _vp, _vp]),
    "lsd_enqueue_pg_vet_device": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _dbl, _vp, _vp]),
    "lsd_pg_marginals": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp, _i, lsd_pg_marg, _vp, _vp]),
    "lsd_pg_vet": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _i, _dbl, _vp]),
    "lsd_pg_append": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, C.c_int32, _vp, _vp, _i, lsd_pg_append, _vp]),
    "lsd_enqueue_pg_describe_device": (_i, [_vp, _vp, _i, _vp, _vp, _i, _dbl, _vp, _vp]),
    "lsd_enqueue_pg_recognize_device": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, lsd_pg_place, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lsd_pg_describe": (_i, [_vp, _vp, _vp, _i, _i, _dbl, _vp]),
    "lsd_pg_recognize": (_i, [_vp, _vp, _i, _i, lsd_pg_place, _vp, _vp]),
    "lsd_enqueue_pg_recognize_all_device": (_i, [_vp, _vp, _i, _vp, lsd_pg_place, _i, _i, _vp, _vp, _vp]),
    "lsd_pg_loops_workspace_bytes": (_sz, [_i, _i, _i]),
    "lsd_enqueue_pg_loops_device": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _i, lsd_pg_loops, _vp, _vp, _vp, _vp]),
    "lsd_enqueue_pg_loop_select_device": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lsd_pg_recognize_all": (_i, [_vp, _vp, _i, _i, _i, lsd_pg_place, _vp, _vp]),
    "lsd_pg_loops": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, lsd_pg_loops, _vp, _vp]),
    "lsd_pg_reduce_workspace_bytes": (_sz, [_i, _i, _i]),
    "lsd_enqueue_pg_reduce_device": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, lsd_pg_reduce, _vp, _vp, _vp, _vp]),
    "lsd_pg_reduce": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, lsd_pg_reduce, _vp, _vp]),
    "lsd_debug_calibrate": (_i, [_vp, _sz]),
    "lsd_debug_eval_math": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _sz]),
    "lsd_debug_lines": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
}
EXPORTED_SYMBOLS = list(_ABI)
del _vp, _i, _sz, _dbl, _pi, _ppar, _localize_args, _live_map_args, _maps_args

_lib = None


def load_library(path=None):
    """Loads liblsdhip.so (built by __graft_entry__.build() / make -C csrc).  Raises if it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("LSD_HIP_LIB") or LIB_PATH      # LSD_HIP_LIB: developer A/B builds
    try:
        # torch bundles its own libamdhip64.so.7; when torch is used in the same process (device buffers,
        # streams, RCCL) it must be the HIP runtime that gets loaded first, or the two runtimes clash.
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(p):
        raise ImportError("liblsdhip.so is not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "-- there is no CPU fallback" % p)
    L = C.CDLL(p)
    # The shipped library exports every symbol (an AttributeError here otherwise); a developer A/B build (LSD_HIP_LIB) may predate any of
    # them and then fails at the call instead.
    for name, (restype, argtypes) in _ABI.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            if not os.environ.get("LSD_HIP_LIB"):
                raise
            continue
        fn.restype, fn.argtypes = restype, argtypes
    if path is None:
        _lib = L
    return L


def shard_range(n_items, world, rank):
    """lsd_shard_range: the contiguous shard [lo, hi) of n_items images that `rank` of `world` takes."""
    lo, hi = C.c_int(), C.c_int()
    load_library().lsd_shard_range(n_items, world, rank, C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def shard_balanced(costs, world):
    """lsd_shard_balanced -> perm int32 [n]: rank r takes images perm[lo_r:hi_r] (shard_range) and every rank carries about the same cost."""
    c = np.ascontiguousarray(costs, np.int64)
    perm = np.zeros(len(c), np.int32)
    st = load_library().lsd_shard_balanced(c.ctypes.data, len(c), world, perm.ctypes.data)
    if st != LSD_OK:
        raise LsdError(st, load_library().lsd_strerror(st).decode())
    return perm


def gather_layout(n_total, world):
    """lsd_gather_layout -> (images of the largest shard, int32 words of the gathered counts array)."""
    per, words = C.c_int(), C.c_size_t()
    st = load_library().lsd_gather_layout(n_total, world, C.byref(per), C.byref(words))
    if st != LSD_OK:
        raise LsdError(st, load_library().lsd_strerror(st).decode())
    return per.value, words.value


def gather_unpack(counts_all, slabs_all, n_total, world, cap_rows):
    """lsd_gather_unpack on HOST copies of the gathered arrays (int32 [world, per + 2], LINE_DTYPE / 80-byte records [world, cap_rows]):
    returns (offsets int32 [n_total + 1], lines LINE_DTYPE in global image order); raises LsdError(LSD_ERR_CAPACITY) if a rank dropped rows
    and LsdError(LSD_ERR_INTERNAL) if the region stage gave an image up -- the exception's `partial` holds what did arrive."""
    L = load_library()
    ca = np.ascontiguousarray(counts_all, np.int32)
    sl = np.ascontiguousarray(slabs_all).view(np.uint8).reshape(-1, 80)
    offs = np.zeros(n_total + 1, np.int32)
    per, _ = gather_layout(n_total, world)
    total = int(ca.reshape(world, per + 2)[:, :per].sum())
    lines = np.zeros(max(total, 1), LINE_DTYPE)
    st = L.lsd_gather_unpack(ca.ctypes.data, sl.ctypes.data, n_total, world, cap_rows, offs.ctypes.data, lines.ctypes.data, len(lines))
    if st in (LSD_ERR_CAPACITY, LSD_ERR_INTERNAL):
        raise LsdError(st, L.lsd_strerror(st).decode(), partial=(offs, lines[:offs[-1]]))
    if st != LSD_OK:
        raise LsdError(st, L.lsd_strerror(st).decode())
    return offs, lines[:offs[-1]]


def make_params(sca=lsd_sca, sig=lsd_sig, angThre=lsd_angThre, denThre=lsd_denThre, pseBin=pseBin):
    return lsd_params(float(sca), float(sig), float(angThre), float(denThre), int(pseBin))


def scaled_size(cols, rows, sca=lsd_sca):
    w, h = C.c_int(), C.c_int()
    load_library().lsd_scaled_size(cols, rows, sca, C.byref(w), C.byref(h))
    return w.value, h.value


class Context:
    """One lsd_ctx: one GPU, one stream, one HBM workspace (one per process rank)."""

    def __init__(self, device=0):
        self.L = load_library()
        h = C.c_void_p()
        st = self.L.lsd_create(C.byref(h), int(device))
        if st != LSD_OK:
            raise LsdError(st, self.L.lsd_strerror(st).decode())
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.L.lsd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, st, allow=(), partial=None):
        if st != LSD_OK and st not in allow:
            raise LsdError(st, self.L.lsd_strerror(st).decode() + " / " + self.L.lsd_last_error(self.h).decode(),
                           partial=partial if st == LSD_ERR_CAPACITY else None)
        return st

    def _take_lines(self, lines_p, n):
        """The n records of the buffer the C side has handed over (run / run_batch) as a LINE_DTYPE array; the buffer is freed, before
        any raise.  The bytes are the device's, the tail padding of structLinesInfo (_pad, which K5 writes as 0) included."""
        lines = np.zeros(n if lines_p else 0, LINE_DTYPE)
        if len(lines):
            C.memmove(lines.ctypes.data, lines_p, 80 * len(lines))
        self.L.lsd_free(lines_p)
        return lines

    # -- host-buffer entry points -----------------------------------------------------------------
    def run(self, map_u8, params=None, want_lineim=True):
        """lsd_run on a C-contiguous uint8 image; the image is rewritten in place like the reference does.  An image with more lines
        than the host capacity (set_host_max_lines) raises LsdError(LSD_ERR_CAPACITY) whose `partial` is what the call would have
        returned: the first records and their raster."""
        assert map_u8.dtype == np.uint8 and map_u8.ndim == 2
        rows, cols = map_u8.shape
        p = params or make_params()
        line_im = np.zeros((rows, cols), np.uint8) if want_lineim else None
        lines_p, n = C.c_void_p(), C.c_int()
        st = self.L.lsd_run(self.h, map_u8.ctypes.data, cols, rows, map_u8.strides[0], C.byref(p),
                            line_im.ctypes.data if want_lineim else None, cols, C.byref(lines_p), C.byref(n))
        lines = self._take_lines(lines_p, n.value)
        self._chk(st, partial=(lines, line_im))
        return lines, line_im

    def run_batch(self, maps_u8, params=None, want_lineim=True):
        """lsd_run_batch on an [n, rows, cols] uint8 array (rewritten in place) -> (lines, offsets int32 [n + 1], line_ims).  On
        LSD_ERR_CAPACITY (an image with more lines than the host capacity: its first records are kept) the raised LsdError's
        `partial` holds that triple."""
        assert maps_u8.dtype == np.uint8 and maps_u8.ndim == 3 and maps_u8.flags.c_contiguous
        n, rows, cols = maps_u8.shape
        p = params or make_params()
        line_ims = np.zeros((n, rows, cols), np.uint8) if want_lineim else None
        lines_p = C.c_void_p()
        offs = (C.c_int * (n + 1))()
        st = self.L.lsd_run_batch(self.h, maps_u8.ctypes.data, n, cols, rows, C.byref(p),
                                  line_ims.ctypes.data if want_lineim else None, C.byref(lines_p), offs)
        offsets = np.frombuffer(offs, np.int32).copy()
        lines = self._take_lines(lines_p, int(offsets[-1]))
        self._chk(st, partial=(lines, offsets, line_ims))
        return lines, offsets, line_ims

    # -- device-resident batch --------------------------------------------------------------------
    def enqueue_device(self, d_maps, n, cols, rows, d_lines, max_lines, d_counts, d_line_ims=None, params=None,
                       flags=0, stream=None):
        """Pointers are raw device addresses (e.g. torch tensor .data_ptr()); asynchronous."""
        p = params or make_params()
        return self._chk(self.L.lsd_enqueue_batch_device(self.h, d_maps, n, cols, rows, C.byref(p), flags, d_line_ims,
                                                         d_lines, max_lines, d_counts, stream))

    def gather_lines(self, comm, d_lines, d_counts, n_local, max_lines, n_total, cap_rows, d_counts_all, d_slabs_all, stream=None):
        """lsd_gather_lines: comm is an lsd_comm (dist.torch_comm / lsd_comm_from_rccl); pointers are raw device addresses."""
        return self._chk(self.L.lsd_gather_lines(self.h, C.byref(comm), d_lines, d_counts, n_local, max_lines, n_total, cap_rows,
                                                 d_counts_all, d_slabs_all, stream))

    def map_cache(self, map_u8, res, z_occ_max_dis=1.0):
        """lsd_map_cache on a uint8 image (read-only); returns float64 [rows, cols]."""
        assert map_u8.dtype == np.uint8 and map_u8.ndim == 2
        rows, cols = map_u8.shape
        out = np.zeros((rows, cols), np.float64)
        self._chk(self.L.lsd_map_cache(self.h, map_u8.ctypes.data, cols, rows, map_u8.strides[0], float(res),
                                       float(z_occ_max_dis), out.ctypes.data))
        return out

    def enqueue_map_cache_device(self, d_maps, n, cols, rows, res, z_occ_max_dis, d_out, stream=None):
        return self._chk(self.L.lsd_enqueue_map_cache_device(self.h, d_maps, n, cols, rows, float(res),
                                                             float(z_occ_max_dis), d_out, stream))

    def scan_to_map_match(self, map_cache, map_lines, scan_lines, scan_im_points, lidar_pose, last_pose, pairs,
                          z_occ=1.0, max_esti_dist=60.0):
        """lsd_scan_to_map_match: map_cache float64 [rows, cols]; lines LINE_DTYPE arrays; scan_im_points POS_DTYPE (or
        [n, 3] float64); poses (x, y[, ang]); pairs int32 [m, 2] = (cntMapLine, cntScanLine).  Returns SCORE_DTYPE [m, 4]."""
        mc = np.ascontiguousarray(map_cache, np.float64)
        rows, cols = mc.shape
        ml = np.ascontiguousarray(map_lines, LINE_DTYPE); sl = np.ascontiguousarray(scan_lines, LINE_DTYPE)
        pts = np.ascontiguousarray(scan_im_points).view(np.float64).reshape(-1, 3)
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        out = np.zeros((len(pr), 4), SCORE_DTYPE)
        self._chk(self.L.lsd_scan_to_map_match(self.h, mc.ctypes.data, cols, rows, ml.ctypes.data, len(ml), sl.ctypes.data, len(sl),
                                               pts.ctypes.data, len(pts), _pos(lidar_pose), _pos(last_pose), pr.ctypes.data, len(pr),
                                               float(z_occ), float(max_esti_dist), out.ctypes.data))
        return out

    def set_scan_capacity(self, readings):
        """lsd_set_scan_capacity: the most readings per scan (the largest stride) FeatureScan, the ingest entries and localize take, 1024
        (the default) .. LSD_SCAN_MAX_LEN = 4096.  Strides above 1024 run on the long FeatureScan kernel, with the same results."""
        self._chk(self.L.lsd_set_scan_capacity(self.h, int(readings)))

    @property
    def scan_capacity(self):
        """lsd_scan_capacity: the context's scan capacity in readings."""
        return int(self.L.lsd_scan_capacity(self.h))

    def feature_scan_batch(self, scans, lens, map_param, region_point_limit=rdp_leastPoint, thre_line=rdp_threLine,
                           line_dist_thre_m=rdp_leastDist, pts_cap=4096):
        """lsd_feature_scan_batch: scans float64 [n, stride, 2] = (range, angle), lens int32 [n] finite readings per scan (stride up to
        the context's scan_capacity: 1024 unless set_scan_capacity raised it),
        map_param = (oriMapCol, oriMapRow, mapResol, mapOriX, mapOriY).  Returns a list of dicts like FeatureScan() below."""
        sc = np.ascontiguousarray(scans, np.float64)
        n, stride = sc.shape[0], sc.shape[1]
        ln = np.ascontiguousarray(lens, np.int32)
        lines = np.zeros((n, 360), LINE_DTYPE); pts = np.zeros((n, pts_cap, 3), np.float64)
        nl = np.zeros(n, np.int32); npt = np.zeros(n, np.int32); lp = np.zeros((n, 2), np.float64); sz = np.zeros((n, 2), np.int32)
        mp = _map_param(map_param)
        # (more than 360 line records in a scan -- the reference would overrun its array there -- raises LsdError(LSD_ERR_CAPACITY), with
        #  the stored records, which the C side says are valid, in the exception's `partial`)
        st = self.L.lsd_feature_scan_batch(self.h, sc.ctypes.data, ln.ctypes.data, n, stride, mp, int(region_point_limit), float(thre_line),
                                           float(line_dist_thre_m), lines.ctypes.data, nl.ctypes.data, pts.ctypes.data, pts_cap,
                                           npt.ctypes.data, lp.ctypes.data, sz.ctypes.data)
        if st != LSD_ERR_CAPACITY:
            self._chk(st)
        out = []
        for i in range(n):
            nl[i] = min(int(nl[i]), 360)
            if npt[i] > pts_cap:
                raise RuntimeError("scan %d marks %d pixels, more than pts_cap" % (i, npt[i]))
            p = pts[i, :npt[i]].copy()
            im = np.zeros((max(int(sz[i, 1]), 0), max(int(sz[i, 0]), 0)), np.uint8)        # FS.lineIm (myRDP.cpp:38, :141)
            if len(p):
                im[p[:, 1].astype(int), p[:, 0].astype(int)] = 255
            out.append(dict(linesInfo=lines[i, :nl[i]].copy(), len_linesInfo=int(nl[i]), scanImPoint=p, lidarPos=(float(lp[i, 0]), float(lp[i, 1])),
                            lineIm=im))
        if st == LSD_ERR_CAPACITY:
            raise LsdError(st, self.L.lsd_strerror(st).decode(), partial=out)
        return out

    def enqueue_scan_ingest_device(self, d_raw, n_scans, n_beams, d_take, d_scans, d_lens, stride, stream=None):
        """lsd_enqueue_scan_ingest_device on device pointers: n_scans x n_beams raw (range, angle) pairs -> d_scans [n_scans, stride, 2]
        (the readings whose range is not +inf first, the rest +0.0) and d_lens; d_take: None, or one int per scan (0: lens 0, row zeroed)."""
        return self._chk(self.L.lsd_enqueue_scan_ingest_device(self.h, d_raw, int(n_scans), int(n_beams), d_take, d_scans, d_lens, int(stride),
                                                               stream))

    def enqueue_laserscan_ingest_device(self, d_ranges, d_angle_min_inc, n_scans, n_beams, d_take, d_scans, d_lens, stride, stream=None):
        """lsd_enqueue_laserscan_ingest_device on device pointers: float32 ranges [n_scans, n_beams] and (angle_min, angle_increment)
        float32 [n_scans, 2] of sensor_msgs/LaserScan messages; the outputs as enqueue_scan_ingest_device."""
        return self._chk(self.L.lsd_enqueue_laserscan_ingest_device(self.h, d_ranges, d_angle_min_inc, int(n_scans), int(n_beams), d_take,
                                                                    d_scans, d_lens, int(stride), stream))

    # -- FeatureAssociation ------------------------------------------------------------------------
    @staticmethod
    def fa_initial_state():
        """lsd_fa_initial_state: the replay driver's starting state (LSD/main_on_windows.cpp:80-93) as an FA_STATE_DTYPE record."""
        st = np.zeros(1, FA_STATE_DTYPE)
        load_library().lsd_fa_initial_state(st.ctypes.data)
        return st[0]

    def feature_association(self, map_cache, map_lines, scan_lines, scan_im_points, lidar_pose, last_pose, scan_pose, state):
        """lsd_feature_association: one frame of myfa::FeatureAssociation.  state: FA_STATE_DTYPE record (or (x [9], P [9, 9]) with P
        indexed P[i, j]).  Returns (state out, report) as FA_STATE_DTYPE / FA_REPORT_DTYPE records."""
        mc = np.ascontiguousarray(map_cache, np.float64)
        rows, cols = mc.shape
        ml, sl = np.ascontiguousarray(map_lines, LINE_DTYPE), np.ascontiguousarray(scan_lines, LINE_DTYPE)
        pts = np.ascontiguousarray(scan_im_points, np.float64).reshape(-1, 3)
        st_in = fa_state(state)
        st_out = np.zeros(1, FA_STATE_DTYPE); rep = np.zeros(1, FA_REPORT_DTYPE)
        self._chk(self.L.lsd_feature_association(self.h, mc.ctypes.data, cols, rows, ml.ctypes.data, len(ml), sl.ctypes.data, len(sl),
                                                 pts.ctypes.data, len(pts), _pos(lidar_pose), _pos(last_pose), _pos(scan_pose),
                                                 st_in.ctypes.data, st_out.ctypes.data, rep.ctypes.data))
        return st_out[0], rep[0]

    def debug_fa_fuse(self, cands, last_pose, scan_pose, state):
        """lsd_debug_fa_fuse: the fusion kernel on a candidate list float64 [n, 4] = (x, y, ang, score) in single-thread order."""
        cd = np.ascontiguousarray(np.asarray(cands, np.float64).reshape(-1, 4))
        st_in = fa_state(state)
        st_out = np.zeros(1, FA_STATE_DTYPE); rep = np.zeros(1, FA_REPORT_DTYPE)
        self._chk(self.L.lsd_debug_fa_fuse(self.h, cd.ctypes.data, len(cd), _pos(last_pose), _pos(scan_pose), st_in.ctypes.data,
                                           st_out.ctypes.data, rep.ctypes.data))
        return st_out[0], rep[0]

    def localize(self, map_cache, map_lines, scans, lens, odom, map_param, init=None):
        """lsd_localize: replays one log.  scans float64 [n, stride, 2] (finite readings first, lens[t] of them), odom float64
        [n + 1, 3] (the reference's Odom vector, load_odom), map_param = (oriMapCol, oriMapRow, mapResol, mapOriX, mapOriY).
        Returns (states FA_STATE_DTYPE [n], reports FA_REPORT_DTYPE [n])."""
        mc = np.ascontiguousarray(map_cache, np.float64)
        rows, cols = mc.shape
        ml = np.ascontiguousarray(map_lines, LINE_DTYPE)
        sc = np.ascontiguousarray(scans, np.float64)
        n, stride = sc.shape[0], sc.shape[1]
        ln = np.ascontiguousarray(lens, np.int32)
        od = np.ascontiguousarray(odom, np.float64).reshape(-1, 3)
        if len(od) != n + 1:
            raise LsdError(LSD_ERR_INVALID, "odom must have one row more than there are frames")
        mp = _map_param(map_param)
        ini = None if init is None else fa_state(init)
        states = np.zeros(n, FA_STATE_DTYPE); reps = np.zeros(n, FA_REPORT_DTYPE)
        self._chk(self.L.lsd_localize(self.h, mc.ctypes.data, cols, rows, ml.ctypes.data, len(ml), sc.ctypes.data, ln.ctypes.data, n, stride,
                                      od.ctypes.data, mp, None if ini is None else ini.ctypes.data, states.ctypes.data, reps.ctypes.data))
        return states, reps

    def enqueue_localize_device(self, d_map_cache, cols, rows, d_map_lines, n_map, n_seq, frames_pitch, n_frames, d_lines, d_n_lines, d_pts,
                                pts_cap, d_n_pts, d_lidar_pos, d_odom, map_resol, d_init, d_states, d_reports, stream=None):
        """lsd_enqueue_localize_device on device pointers; n_frames: host int sequence [n_seq]."""
        nf = np.ascontiguousarray(n_frames, np.int32)
        return self._chk(self.L.lsd_enqueue_localize_device(self.h, d_map_cache, cols, rows, d_map_lines, n_map, n_seq, frames_pitch,
                                                            nf.ctypes.data, d_lines, d_n_lines, d_pts, pts_cap, d_n_pts, d_lidar_pos, d_odom,
                                                            float(map_resol), d_init, d_states, d_reports, stream))

    @staticmethod
    def fa_carry_init(state=None, odom0=(0.0, 0.0, 0.0)):
        """lsd_fa_carry_init: the loop's variables before the driver's first frame as an FA_CARRY_DTYPE record: state (None: the
        initial state), Odom[0] = odom0 (the driver's Odom[0].x is 0), no angle offsets, frames = 0."""
        c = np.zeros(1, FA_CARRY_DTYPE)
        st = None if state is None else fa_state(state)
        load_library().lsd_fa_carry_init(c.ctypes.data, None if st is None else st.ctypes.data, _pos(odom0))
        return c[0]

    def enqueue_localize_resume_device(self, d_map_cache, cols, rows, d_map_lines, n_map, n_seq, frames_pitch, n_frames, d_lines, d_n_lines,
                                       d_pts, pts_cap, d_n_pts, d_lidar_pos, d_odom, map_resol, d_carry, d_states, d_reports, stream=None):
        """lsd_enqueue_localize_resume_device on device pointers; n_frames: host int sequence [n_seq]; d_odom: n_seq x frames_pitch NEW
        odometry rows; d_carry: n_seq FA_CARRY_DTYPE records, read and updated in place."""
        nf = np.ascontiguousarray(n_frames, np.int32)
        return self._chk(self.L.lsd_enqueue_localize_resume_device(self.h, d_map_cache, cols, rows, d_map_lines, n_map, n_seq, frames_pitch,
                                                                   nf.ctypes.data, d_lines, d_n_lines, d_pts, pts_cap, d_n_pts, d_lidar_pos,
                                                                   d_odom, float(map_resol), d_carry, d_states, d_reports, stream))

    def enqueue_localize_live_map_device(self, d_map_cache, cols, rows, d_map_lines, map_lines_cap, d_n_map, n_seq, frames_pitch, n_frames,
                                         d_lines, d_n_lines, d_pts, pts_cap, d_n_pts, d_lidar_pos, d_odom, map_resol, d_init, d_states,
                                         d_reports, stream=None):
        """lsd_enqueue_localize_live_map_device: enqueue_localize_device with the map's line count read on the device (d_n_map: one
        int32, held to 0..map_lines_cap; d_map_lines: map_lines_cap records)."""
        nf = np.ascontiguousarray(n_frames, np.int32)
        return self._chk(self.L.lsd_enqueue_localize_live_map_device(self.h, d_map_cache, cols, rows, d_map_lines, map_lines_cap, d_n_map,
                                                                     n_seq, frames_pitch, nf.ctypes.data, d_lines, d_n_lines, d_pts, pts_cap,
                                                                     d_n_pts, d_lidar_pos, d_odom, float(map_resol), d_init, d_states,
                                                                     d_reports, stream))

    def enqueue_localize_resume_live_map_device(self, d_map_cache, cols, rows, d_map_lines, map_lines_cap, d_n_map, n_seq, frames_pitch,
                                                n_frames, d_lines, d_n_lines, d_pts, pts_cap, d_n_pts, d_lidar_pos, d_odom, map_resol,
                                                d_carry, d_states, d_reports, stream=None):
        """lsd_enqueue_localize_resume_live_map_device: enqueue_localize_resume_device with the map's line count read on the device."""
        nf = np.ascontiguousarray(n_frames, np.int32)
        return self._chk(self.L.lsd_enqueue_localize_resume_live_map_device(self.h, d_map_cache, cols, rows, d_map_lines, map_lines_cap,
                                                                            d_n_map, n_seq, frames_pitch, nf.ctypes.data, d_lines, d_n_lines,
                                                                            d_pts, pts_cap, d_n_pts, d_lidar_pos, d_odom, float(map_resol),
                                                                            d_carry, d_states, d_reports, stream))

    def enqueue_feature_scan_maps_device(self, d_scans, d_lens, n_scans, stride, maps, d_map_of, scans_per_seq, d_lines_out, d_n_lines,
                                         d_pts_out, pts_cap, d_n_pts, d_lidar_pos, d_im_size, region_point_limit=rdp_leastPoint,
                                         thre_line=rdp_threLine, line_dist_thre_m=rdp_leastDist, stream=None):
        """lsd_enqueue_feature_scan_maps_device on device pointers: FeatureScan of n_scans scans, scan i with mapResol / mapOriX / mapOriY
        of map d_map_of[i // scans_per_seq].  maps: a HOST table (map_table); d_map_of: device int32, one id per sequence, an id outside
        the table: the sequence's scans get counts 0 and nothing else."""
        tab = map_table(maps)
        return self._chk(self.L.lsd_enqueue_feature_scan_maps_device(self.h, d_scans, d_lens, int(n_scans), int(stride), tab.ctypes.data,
                                                                     len(tab), d_map_of, int(scans_per_seq), int(region_point_limit),
                                                                     float(thre_line), float(line_dist_thre_m), d_lines_out, d_n_lines,
                                                                     d_pts_out, int(pts_cap), d_n_pts, d_lidar_pos, d_im_size, stream))

    def enqueue_localize_maps_device(self, maps, d_map_of, n_seq, frames_pitch, n_frames, d_lines, d_n_lines, d_pts, pts_cap, d_n_pts,
                                     d_lidar_pos, d_odom, d_init, d_states, d_reports, stream=None):
        """lsd_enqueue_localize_maps_device: enqueue_localize_device with sequence s against map d_map_of[s] of the HOST table `maps`
        (map_table); an id outside the table: the sequence sits the call out."""
        tab, nf = map_table(maps), np.ascontiguousarray(n_frames, np.int32)
        return self._chk(self.L.lsd_enqueue_localize_maps_device(self.h, tab.ctypes.data, len(tab), d_map_of, int(n_seq), int(frames_pitch),
                                                                 nf.ctypes.data, d_lines, d_n_lines, d_pts, int(pts_cap), d_n_pts, d_lidar_pos,
                                                                 d_odom, d_init, d_states, d_reports, stream))

    def enqueue_localize_resume_maps_device(self, maps, d_map_of, n_seq, frames_pitch, n_frames, d_lines, d_n_lines, d_pts, pts_cap, d_n_pts,
                                            d_lidar_pos, d_odom, d_carry, d_states, d_reports, stream=None):
        """lsd_enqueue_localize_resume_maps_device: enqueue_localize_resume_device with sequence s against map d_map_of[s]."""
        tab, nf = map_table(maps), np.ascontiguousarray(n_frames, np.int32)
        return self._chk(self.L.lsd_enqueue_localize_resume_maps_device(self.h, tab.ctypes.data, len(tab), d_map_of, int(n_seq),
                                                                        int(frames_pitch), nf.ctypes.data, d_lines, d_n_lines, d_pts,
                                                                        int(pts_cap), d_n_pts, d_lidar_pos, d_odom, d_carry, d_states,
                                                                        d_reports, stream))

    def enqueue_fa_carry_rebase_device(self, d_carry, n_seq, d_key, key, frame_from, frame_to, stream=None):
        """lsd_enqueue_fa_carry_rebase_device: the n_seq carries at d_carry (FA_CARRY_DTYPE records on the device) from the map frame
        frame_from to frame_to (map_frame: (mapResol, mapOriX, mapOriY), or a map_param), in place, asynchronous on `stream`.  d_key: None
        (every sequence), or device int32 [n_seq]: sequence s moves iff d_key[s] == key, read when the kernel runs.  The arguments the
        C entry refuses are refused here first, before the library is called."""
        f, t = map_frame(frame_from), map_frame(frame_to)
        if not d_carry or int(n_seq) <= 0:
            raise LsdError(LSD_ERR_INVALID, "a null carry, or n_seq <= 0")
        return self._chk(self.L.lsd_enqueue_fa_carry_rebase_device(self.h, d_carry, int(n_seq), d_key, int(key), f, t, stream))

    def enqueue_fa_carry_correct_device(self, d_carry, n_seq, frames_pitch, d_poses, pose_pitch, d_resp, d_key=None, key=0, correct=None,
                                        d_rep=None, stream=None):
        """lsd_enqueue_fa_carry_correct_device: the grid match response fused into the n_seq carries at d_carry, in place,
        asynchronous on `stream`, on raw device addresses.  Per sequence: the frames_pitch ORIGINAL poses of its slots (the first 24 bytes
        of the records at d_poses, pose_pitch apart: the poses the match was given) and its response records at d_resp
        (GRID_RESPONSE_DTYPE); the slot whose pose equals the carry's, byte for byte, is the one fused.  d_key: None (every sequence), or
        device int32 [n_seq]: sequence s takes part iff d_key[s] == key, read when the kernel runs.  correct: fa_correct().  d_rep: None,
        or n_seq reports of FA_CORRECT_DTYPE."""
        return self._chk(self.L.lsd_enqueue_fa_carry_correct_device(self.h, d_carry, int(n_seq), int(frames_pitch), d_poses, int(pose_pitch),
                                                                    d_resp, d_key, int(key), fa_correct(correct), d_rep, stream))

    def fa_carry_correct(self, carries, poses, resp, correct=None):
        """lsd_fa_carry_correct from host arrays: carries FA_CARRY_DTYPE [n_seq], poses float64 [n_seq, frames_pitch, 3] (the poses the match
        was given), resp GRID_RESPONSE_DTYPE [n_seq, frames_pitch].  Returns (the carries after the update, the reports: FA_CORRECT_DTYPE
        [n_seq]); the arguments are not modified.  Blocking."""
        cy = np.array(carries, FA_CARRY_DTYPE).reshape(-1)
        po = np.ascontiguousarray(poses, np.float64)
        rs = np.ascontiguousarray(resp)
        if po.ndim != 3 or po.shape[0] != len(cy) or po.shape[2] != 3 or rs.dtype != GRID_RESPONSE_DTYPE or rs.shape != po.shape[:2]:
            raise LsdError(LSD_ERR_INVALID, "carries FA_CARRY_DTYPE [n], poses [n, frames_pitch, 3], resp GRID_RESPONSE_DTYPE [n, frames_pitch]")
        rep = np.zeros(len(cy), FA_CORRECT_DTYPE)
        self._chk(self.L.lsd_fa_carry_correct(self.h, cy.ctypes.data, len(cy), po.shape[1], po.ctypes.data, rs.ctypes.data, fa_correct(correct),
                                              rep.ctypes.data))
        return cy, rep

    # -- relocalisation: gather the lost, (locate,) seed the carries (k_falost.hip, k_faseed.hip) --
    def enqueue_fa_lost_gather_device(self, d_carry, n_seq, frames_pitch, d_poses, pose_pitch, d_scans, d_lens, stride, d_key, key, max_lost,
                                      d_scans_out, d_lens_out, d_pick, d_n_lost, stream=None):
        """lsd_enqueue_fa_lost_gather_device on raw device addresses: the sequences without a pose whose tick had a scan (d_key: None, or
        device int32 [n_seq] with sequence s taking part iff d_key[s] == key) take ranks in ascending s; the first max_lost have their slot
        written to d_pick (int32 [max_lost], -1 beyond), their scan row copied to d_scans_out ([max_lost, stride, 2] doubles) and its length
        to d_lens_out (0 beyond); d_n_lost: int32 [2], the number lost and the number gathered.  Asynchronous on `stream`."""
        return self._chk(self.L.lsd_enqueue_fa_lost_gather_device(self.h, d_carry, int(n_seq), int(frames_pitch), d_poses, int(pose_pitch), d_scans,
                                                                  d_lens, int(stride), d_key, int(key), int(max_lost), d_scans_out, d_lens_out,
                                                                  d_pick, d_n_lost, stream))

    def fa_lost_gather(self, carries, poses, scans, lens, max_lost, scans_out=None):
        """lsd_fa_lost_gather from host arrays: carries FA_CARRY_DTYPE [n_seq], poses float64 [n_seq, frames_pitch, 3], scans float64 [n_seq,
        frames_pitch, stride, 2], lens int32 [n_seq, frames_pitch]; scans_out (float64 [max_lost, stride, 2]; None: zeros) is what the rows
        past the gathered ones keep.  Returns (scans_out, lens_out int32 [max_lost], pick int32 [max_lost], n_lost int32 [2]); the arguments
        are not modified.  Blocking."""
        cy = np.ascontiguousarray(carries, FA_CARRY_DTYPE).reshape(-1)
        po, sc, ln = np.ascontiguousarray(poses, np.float64), np.ascontiguousarray(scans, np.float64), np.ascontiguousarray(lens, np.int32)
        n = int(max_lost)
        if (po.ndim != 3 or po.shape[0] != len(cy) or po.shape[2] != 3 or sc.ndim != 4 or sc.shape[:2] != po.shape[:2] or sc.shape[3] != 2 or
                ln.shape != po.shape[:2] or not 1 <= n <= 4096):
            raise LsdError(LSD_ERR_INVALID, "carries [n], poses [n, frames_pitch, 3], scans [n, frames_pitch, stride, 2], lens [n, frames_pitch], "
                                            "max_lost 1..4096")
        so = np.zeros((n, sc.shape[2], 2)) if scans_out is None else np.array(scans_out, np.float64)
        if so.shape != (n, sc.shape[2], 2):
            raise LsdError(LSD_ERR_INVALID, "scans_out must be [max_lost, stride, 2]")
        lo, pk, nl = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(2, np.int32)
        self._chk(self.L.lsd_fa_lost_gather(self.h, cy.ctypes.data, len(cy), po.shape[1], po.ctypes.data, sc.ctypes.data, ln.ctypes.data, sc.shape[2],
                                            n, so.ctypes.data, lo.ctypes.data, pk.ctypes.data, nl.ctypes.data))
        return so, lo, pk, nl

    def enqueue_fa_carry_seed_device(self, d_carry, n_seq, frames_pitch, d_pick, n_pick, d_loc, d_resp=None, seed=None, d_rep=None, stream=None):
        """lsd_enqueue_fa_carry_seed_device on raw device addresses: for each of the n_pick slots of d_pick (the gather's) whose carry still
        has no pose, whose locate record at d_loc (GRID_LOCATE_DTYPE) is accepted and names at most seed.max_best equal winners, the carry
        becomes the located pose -- d_resp (GRID_RESPONSE_DTYPE [n_pick]) given: the response's, with its covariance -- at rest, and the
        loop's angle bookkeeping the one offset a first frame there would push.  seed: fa_seed().  d_rep: None, or n_pick reports of
        FA_SEED_DTYPE.  Asynchronous on `stream`."""
        return self._chk(self.L.lsd_enqueue_fa_carry_seed_device(self.h, d_carry, int(n_seq), int(frames_pitch), d_pick, int(n_pick), d_loc, d_resp,
                                                                 fa_seed(seed), d_rep, stream))

    def fa_carry_seed(self, carries, frames_pitch, pick, loc, resp=None, seed=None):
        """lsd_fa_carry_seed from host arrays: carries FA_CARRY_DTYPE [n_seq], pick int32 [n_pick], loc GRID_LOCATE_DTYPE [n_pick], resp None or
        GRID_RESPONSE_DTYPE [n_pick].  Returns (the carries after, the reports: FA_SEED_DTYPE [n_pick]); the arguments are not modified.
        Blocking."""
        cy = np.array(carries, FA_CARRY_DTYPE).reshape(-1)
        pk, lc = np.ascontiguousarray(pick, np.int32).reshape(-1), np.ascontiguousarray(loc)
        rs = None if resp is None else np.ascontiguousarray(resp)
        if lc.dtype != GRID_LOCATE_DTYPE or lc.shape != pk.shape or (rs is not None and (rs.dtype != GRID_RESPONSE_DTYPE or rs.shape != pk.shape)):
            raise LsdError(LSD_ERR_INVALID, "pick int32 [n], loc GRID_LOCATE_DTYPE [n], resp None or GRID_RESPONSE_DTYPE [n]")
        rep = np.zeros(len(pk), FA_SEED_DTYPE)
        self._chk(self.L.lsd_fa_carry_seed(self.h, cy.ctypes.data, len(cy), int(frames_pitch), pk.ctypes.data, len(pk), lc.ctypes.data,
                                           None if rs is None else rs.ctypes.data, fa_seed(seed), rep.ctypes.data))
        return cy, rep

    # -- the pose graph: keyframes, the loop candidate, the closure edge, the relaxation (k_pgbuild.hip, k_posegraph.hip) --
    def enqueue_pg_append_device(self, d_scans, d_lens, n_cand, stride, d_poses, pose_pitch, d_head, d_nodes, nodes_cap, d_edges, edges_cap,
                                 d_track, track, d_store, d_store_lens, store_stride, append=None, d_rep=None, stream=None):
        """lsd_enqueue_pg_append_device on raw device addresses: n_cand candidate frames (scans, lengths, stride and poses at a pitch as
        enqueue_grid_integrate_device reads them) decided in order against the track record at d_track; a keyframe becomes a node, its
        scan a row of the store, the motion since the last one an edge.  append: pg_append().  d_rep: None, or one PG_APPEND_REP_DTYPE.
        Asynchronous on `stream`."""
        return self._chk(self.L.lsd_enqueue_pg_append_device(self.h, d_scans, d_lens, int(n_cand), int(stride), d_poses, int(pose_pitch), d_head,
                                                             d_nodes, int(nodes_cap), d_edges, int(edges_cap), d_track, int(track), d_store,
                                                             d_store_lens, int(store_stride), pg_append(append), d_rep, stream))

    def enqueue_pg_near_device(self, d_head, d_nodes, nodes_cap, d_track, d_store, d_store_lens, store_stride, gap, radius, window, d_rec, d_sel,
                               d_q_scan, d_q_len, d_q_pose, stream=None):
        """lsd_enqueue_pg_near_device on raw device addresses: the loop candidate of the track's last node -- the nearest node at least
        `gap` indices back and within `radius` pixels -- into d_rec (PG_NEAR_DTYPE), the poses of the nodes within `window` of it into
        d_sel (float64 [nodes_cap, 3], the "no pose" sentinel elsewhere) and the query's scan, length and pose into a batch of one row.
        Asynchronous on `stream`."""
        return self._chk(self.L.lsd_enqueue_pg_near_device(self.h, d_head, d_nodes, int(nodes_cap), d_track, d_store, d_store_lens,
                                                           int(store_stride), int(gap), float(radius), int(window), d_rec, d_sel, d_q_scan, d_q_len,
                                                           d_q_pose, stream))

    def enqueue_pg_closure_device(self, d_head, d_nodes, nodes_cap, d_edges, edges_cap, d_near, d_resp, closure=None, d_rep=None, stream=None):
        """lsd_enqueue_pg_closure_device on raw device addresses: the edge (anchor, query) from the near record and the response record
        (GRID_RESPONSE_DTYPE) of the query matched against the anchor's neighbourhood.  closure: pg_closure().  d_rep: None, or one
        PG_CLOSURE_REP_DTYPE.  Asynchronous on `stream`."""
        return self._chk(self.L.lsd_enqueue_pg_closure_device(self.h, d_head, d_nodes, int(nodes_cap), d_edges, int(edges_cap), d_near, d_resp,
                                                              pg_closure(closure), d_rep, stream))

    def enqueue_pg_relax_device(self, n_graphs, d_heads, d_nodes, nodes_cap, d_edges, edges_cap, d_workspace, d_rep, relax=None, stream=None):
        """lsd_enqueue_pg_relax_device on raw device addresses: n_graphs graphs (heads [n_graphs], nodes [n_graphs, nodes_cap], edges
        [n_graphs, edges_cap], n_graphs x pg_workspace_bytes(nodes_cap, edges_cap) bytes of workspace) relaxed in one launch, one
        workgroup each; the nodes' poses in place, edge.chi2, one PG_RELAX_REP_DTYPE per graph.  relax: pg_relax().  Asynchronous."""
        return self._chk(self.L.lsd_enqueue_pg_relax_device(self.h, int(n_graphs), d_heads, d_nodes, int(nodes_cap), d_edges, int(edges_cap),
                                                            pg_relax(relax), d_workspace, d_rep, stream))

    def pg_relax(self, nodes, edges, relax=None):
        """lsd_pg_relax from host arrays: nodes PG_NODE_DTYPE [n], edges PG_EDGE_DTYPE [m].  Returns (nodes, edges, report) after the
        relaxation; the arguments are not modified.  Blocking."""
        no, ed = np.array(nodes, PG_NODE_DTYPE).reshape(-1), np.array(edges, PG_EDGE_DTYPE).reshape(-1)
        rep = np.zeros(1, PG_RELAX_REP_DTYPE)
        self._chk(self.L.lsd_pg_relax(self.h, no.ctypes.data if len(no) else None, len(no), ed.ctypes.data if len(ed) else None, len(ed),
                                      pg_relax(relax), rep.ctypes.data))
        return no, ed, rep[0]

    def enqueue_pg_relax_robust_device(self, n_graphs, d_heads, d_nodes, nodes_cap, d_edges, edges_cap, d_workspace, d_rep, robust, d_rob_rep=None,
                                       relax=None, stream=None):
        """lsd_enqueue_pg_relax_robust_device on raw device addresses: enqueue_pg_relax_device with a robust kernel on the edges (robust:
        pg_robust()) -- an edge in scope pulls with a weight made from its own chi2, and the objective is the kernel's cost.  edge.chi2
        stays the plain value.  d_rob_rep: None, or one PG_ROBUST_REP_DTYPE per graph.  Asynchronous on `stream`."""
        return self._chk(self.L.lsd_enqueue_pg_relax_robust_device(self.h, int(n_graphs), d_heads, d_nodes, int(nodes_cap), d_edges, int(edges_cap),
                                                                   pg_relax(relax), pg_robust(robust), d_workspace, d_rep, d_rob_rep, stream))

    def enqueue_pg_prune_device(self, n_graphs, d_heads, d_edges, edges_cap, d_rep, gate, max_reject=8, stream=None):
        """lsd_enqueue_pg_prune_device on raw device addresses: in every graph the closure edges that are not disabled and whose chi2
        is not <= gate are candidates; the max_reject (0..64) largest become DISABLED | REJECTED.  One PG_PRUNE_REP_DTYPE per graph.
        Asynchronous on `stream`."""
        mr = int(max_reject)
        if not -2 ** 31 <= mr < 2 ** 31:
            raise LsdError(LSD_ERR_INVALID, "max_reject is int32")
        return self._chk(self.L.lsd_enqueue_pg_prune_device(self.h, int(n_graphs), d_heads, d_edges, int(edges_cap), lsd_pg_prune(float(gate), mr, 0),
                                                            d_rep, stream))

    def pg_relax_robust(self, nodes, edges, robust, relax=None):
        """lsd_pg_relax_robust from host arrays, as pg_relax(): returns (nodes, edges, report, robust report) after the relaxation with
        the kernel `robust` (pg_robust()); blocking."""
        no, ed = np.array(nodes, PG_NODE_DTYPE).reshape(-1), np.array(edges, PG_EDGE_DTYPE).reshape(-1)
        rep, rob = np.zeros(1, PG_RELAX_REP_DTYPE), np.zeros(1, PG_ROBUST_REP_DTYPE)
        self._chk(self.L.lsd_pg_relax_robust(self.h, no.ctypes.data if len(no) else None, len(no), ed.ctypes.data if len(ed) else None, len(ed),
                                             pg_relax(relax), pg_robust(robust), rep.ctypes.data, rob.ctypes.data))
        return no, ed, rep[0], rob[0]

    def enqueue_pg_relax_pc_device(self, n_graphs, d_heads, d_nodes, nodes_cap, d_edges, edges_cap, d_workspace, d_rep, precond, robust=None,
                                   d_rob_rep=None, d_pc_rep=None, relax=None, stream=None):
        """lsd_enqueue_pg_relax_pc_device on raw device addresses: enqueue_pg_relax_robust_device with a choice of preconditioner
        (precond: pg_precond(); robust: pg_robust(), None is the kernel "none").  "block" gives the robust entry's bytes; "chain" solves
        the block-tridiagonal part of the normal matrix along the odometry chains, so that PCG's steps follow the number of closures and
        not the length of the track.  The workspace is n_graphs x pg_workspace_pc_bytes(nodes_cap, edges_cap, precond) bytes.  d_rob_rep,
        d_pc_rep: None, or one PG_ROBUST_REP_DTYPE / PG_PRECOND_REP_DTYPE per graph.  Asynchronous on `stream`."""
        rob = pg_robust(kernel="none") if robust is None else pg_robust(robust)
        return self._chk(self.L.lsd_enqueue_pg_relax_pc_device(self.h, int(n_graphs), d_heads, d_nodes, int(nodes_cap), d_edges, int(edges_cap),
                                                               pg_relax(relax), rob, pg_precond(precond), d_workspace, d_rep, d_rob_rep, d_pc_rep,
                                                               stream))

    def pg_relax_pc(self, nodes, edges, precond, robust=None, relax=None):
        """lsd_pg_relax_pc from host arrays, as pg_relax_robust(): returns (nodes, edges, report, robust report, preconditioner's
        report) after the relaxation preconditioned as `precond` says (pg_precond()); blocking."""
        no, ed = np.array(nodes, PG_NODE_DTYPE).reshape(-1), np.array(edges, PG_EDGE_DTYPE).reshape(-1)
        rep, rob, pc = np.zeros(1, PG_RELAX_REP_DTYPE), np.zeros(1, PG_ROBUST_REP_DTYPE), np.zeros(1, PG_PRECOND_REP_DTYPE)
        rb = pg_robust(kernel="none") if robust is None else pg_robust(robust)
        self._chk(self.L.lsd_pg_relax_pc(self.h, no.ctypes.data if len(no) else None, len(no), ed.ctypes.data if len(ed) else None, len(ed),
                                         pg_relax(relax), rb, pg_precond(precond), rep.ctypes.data, rob.ctypes.data, pc.ctypes.data))
        return no, ed, rep[0], rob[0], pc[0]

    def enqueue_pg_marginals_device(self, d_head, d_nodes, nodes_cap, d_edges, edges_cap, d_queries, n_q, d_workspace, d_recs, d_rep, marg=None,
                                    d_prior=None, stream=None):
        """lsd_enqueue_pg_marginals_device on raw device addresses: the covariance of a node (PG_MARG_NODE), of one node relative to
        another (PG_MARG_PAIR) or of the two ends of the k-th edge appended since the head was copied to d_prior (PG_MARG_NEW_EDGE),
        one PG_MARG_QUERY_DTYPE -> one PG_MARG_REC_DTYPE each, and one PG_MARG_REP_DTYPE; the graph is not changed.  marg: pg_marg().
        The workspace is pg_marginals_workspace_bytes(nodes_cap, edges_cap, precond, slots) bytes.  Asynchronous on `stream`."""
        return self._chk(self.L.lsd_enqueue_pg_marginals_device(self.h, d_head, d_nodes, int(nodes_cap), d_edges, int(edges_cap), d_prior, d_queries,
                                                                int(n_q), pg_marg(marg), d_workspace, d_recs, d_rep, stream))

    def enqueue_pg_vet_device(self, d_head, d_nodes, nodes_cap, d_edges, edges_cap, d_queries, d_recs, n_q, gate, d_rep=None, stream=None):
        """lsd_enqueue_pg_vet_device on raw device addresses: every PG_MARG_NEW_EDGE query whose closure's error at the current poses
        is not plausible under its record's covariance plus the edge's own (!(d2 <= gate)) becomes DISABLED | REJECTED.  d_rep: None,
        or one PG_VET_REP_DTYPE per query.  Asynchronous on `stream`."""
        return self._chk(self.L.lsd_enqueue_pg_vet_device(self.h, d_head, d_nodes, int(nodes_cap), d_edges, int(edges_cap), d_queries, d_recs,
                                                          int(n_q), float(gate), d_rep, stream))

    def pg_marginals(self, nodes, edges, queries, marg=None, prior_edges=-1):
        """lsd_pg_marginals from host arrays: returns (records PG_MARG_REC_DTYPE [n_q], report PG_MARG_REP_DTYPE); blocking.  queries:
        pg_queries().  prior_edges < 0: no prior head."""
        no, ed = np.array(nodes, PG_NODE_DTYPE).reshape(-1), np.array(edges, PG_EDGE_DTYPE).reshape(-1)
        qu = pg_queries(queries)
        recs, rep = np.zeros(len(qu), PG_MARG_REC_DTYPE), np.zeros(1, PG_MARG_REP_DTYPE)
        self._chk(self.L.lsd_pg_marginals(self.h, no.ctypes.data if len(no) else None, len(no), ed.ctypes.data if len(ed) else None, len(ed),
                                          int(prior_edges), qu.ctypes.data if len(qu) else None, len(qu), pg_marg(marg),
                                          recs.ctypes.data if len(qu) else None, rep.ctypes.data))
        return recs, rep[0]

    def pg_vet(self, nodes, edges, queries, recs, gate):
        """lsd_pg_vet from host arrays: returns (edges, reports PG_VET_REP_DTYPE [n_q]) -- the edges with the rejected closures
        flagged; blocking."""
        no, ed = np.array(nodes, PG_NODE_DTYPE).reshape(-1), np.array(edges, PG_EDGE_DTYPE).reshape(-1)
        qu, rc = pg_queries(queries), np.array(recs, PG_MARG_REC_DTYPE).reshape(-1)
        if len(rc) != len(qu):
            raise LsdError(LSD_ERR_INVALID, "one record per query")
        reps = np.zeros(len(qu), PG_VET_REP_DTYPE)
        self._chk(self.L.lsd_pg_vet(self.h, no.ctypes.data if len(no) else None, len(no), ed.ctypes.data if len(ed) else None, len(ed),
                                    qu.ctypes.data if len(qu) else None, rc.ctypes.data if len(qu) else None, len(qu), float(gate),
                                    reps.ctypes.data if len(qu) else None))
        return ed, reps

    def pg_append(self, scans, lens, poses, head, nodes, edges, track_rec, store, store_lens, track=0, append=None):
        """lsd_pg_append from host arrays: the candidates (scans float64 [n, stride, 2], lens int32 [n], poses float64 [n, 3]) against the
        graph head (PG_HEAD_DTYPE), nodes [nodes_cap], edges [edges_cap], track_rec (PG_TRACK_DTYPE), store float64 [nodes_cap,
        store_stride, 2], store_lens int32 [nodes_cap].  Returns (head, nodes, edges, track_rec, store, store_lens, report): new arrays.
        Blocking."""
        sc, ln, po, ok = _host_scans(scans, lens, poses)
        hd, no, ed = np.array(head, PG_HEAD_DTYPE).reshape(1), np.array(nodes, PG_NODE_DTYPE).reshape(-1), np.array(edges, PG_EDGE_DTYPE).reshape(-1)
        tr, st, sl = np.array(track_rec, PG_TRACK_DTYPE).reshape(1), np.array(store, np.float64), np.array(store_lens, np.int32).reshape(-1)
        if not ok or st.ndim != 3 or st.shape[0] != len(no) or st.shape[2] != 2 or len(sl) != len(no):
            raise LsdError(LSD_ERR_INVALID, "scans [n, stride, 2], lens [n], poses [n, 3], store [nodes_cap, store_stride, 2], store_lens [nodes_cap]")
        rep = np.zeros(1, PG_APPEND_REP_DTYPE)
        self._chk(self.L.lsd_pg_append(self.h, sc.ctypes.data, ln.ctypes.data, len(ln), max(sc.shape[1], 0), po.ctypes.data, hd.ctypes.data,
                                       no.ctypes.data, len(no), ed.ctypes.data, len(ed), tr.ctypes.data, int(track), st.ctypes.data, sl.ctypes.data,
                                       st.shape[1], pg_append(append), rep.ctypes.data))
        return hd[0], no, ed, tr[0], st, sl, rep[0]

    def enqueue_pg_describe_device(self, d_head, nodes_cap, d_store, d_store_lens, store_stride, range_max, d_desc, stream=None):
        """lsd_enqueue_pg_describe_device on raw device addresses: every keyframe below n_nodes whose record in d_desc (PG_DESC_DTYPE
        [nodes_cap]) has valid == 0 gets its 64-sector descriptor; the others keep their bytes.  Asynchronous."""
        return self._chk(self.L.lsd_enqueue_pg_describe_device(self.h, d_head, int(nodes_cap), d_store, d_store_lens, int(store_stride), float(range_max),
                                                               d_desc, stream))

    def enqueue_pg_recognize_device(self, d_head, d_nodes, nodes_cap, d_track, d_store, d_store_lens, store_stride, d_desc, place, d_work, d_recs, d_rep,
                                    d_near, d_sel, d_q_scan, d_q_len, d_q_pose, stream=None):
        """lsd_enqueue_pg_recognize_device on raw device addresses: the track's last node scored against every old keyframe's descriptor at
        every circular shift; the best distinct places into d_recs (PG_PLACE_REC_DTYPE [k]) and d_rep (PG_PLACE_REP_DTYPE); the place of
        round `pick` leaves what enqueue_pg_near_device leaves, with the anchor's pose turned by the shift as the query's.  place:
        pg_place(); d_work: nodes_cap uint32.  Asynchronous."""
        return self._chk(self.L.lsd_enqueue_pg_recognize_device(self.h, d_head, d_nodes, int(nodes_cap), d_track, d_store, d_store_lens, int(store_stride),
                                                                d_desc, pg_place(place), d_work, d_recs, d_rep, d_near, d_sel, d_q_scan, d_q_len,
                                                                d_q_pose, stream))

    def pg_describe(self, scans, lens, range_max):
        """lsd_pg_describe from host arrays: scans float64 [n, stride, 2], lens int32 [n] -> PG_DESC_DTYPE [n].  Blocking."""
        sc, ln = np.ascontiguousarray(scans, np.float64), np.ascontiguousarray(lens, np.int32).reshape(-1)
        if sc.ndim != 3 or sc.shape[0] != len(ln) or sc.shape[2] != 2:
            raise LsdError(LSD_ERR_INVALID, "scans [n, stride, 2], lens [n]")
        out = np.zeros(len(ln), PG_DESC_DTYPE)
        self._chk(self.L.lsd_pg_describe(self.h, sc.ctypes.data if len(ln) else None, ln.ctypes.data if len(ln) else None, len(ln), sc.shape[1],
                                         float(range_max), out.ctypes.data if len(ln) else None))
        return out

    def pg_recognize(self, desc, query, place=None):
        """lsd_pg_recognize from host arrays: desc PG_DESC_DTYPE [n] and the query's index -> (records PG_PLACE_REC_DTYPE [k], report
        PG_PLACE_REP_DTYPE); no selection and no gather.  place: pg_place().  Blocking."""
        de, par = np.ascontiguousarray(desc, PG_DESC_DTYPE).reshape(-1), pg_place(place)
        recs, rep = np.zeros(min(max(int(par.k), 1), PG_PLACE_MAX), PG_PLACE_REC_DTYPE), np.zeros(1, PG_PLACE_REP_DTYPE)
        self._chk(self.L.lsd_pg_recognize(self.h, de.ctypes.data if len(de) else None, len(de), int(query), par, recs.ctypes.data, rep.ctypes.data))
        return recs, rep[0]

    def enqueue_pg_recognize_all_device(self, d_head, nodes_cap, d_desc, place, q_lo, n_q, d_recs, d_reps, stream=None):
        """lsd_enqueue_pg_recognize_all_device on raw device addresses: the keyframes q_lo .. q_lo + n_q - 1 as queries in one launch;
        d_recs (PG_PLACE_REC_DTYPE [n_q, k]) and d_reps (PG_PLACE_REP_DTYPE [n_q]) receive, per query, the bytes
        enqueue_pg_recognize_device writes for it.  place: pg_place().  Asynchronous."""
        return self._chk(self.L.lsd_enqueue_pg_recognize_all_device(self.h, d_head, int(nodes_cap), d_desc, pg_place(place), int(q_lo), int(n_q), d_recs,
                                                                    d_reps, stream))

    def enqueue_pg_loops_device(self, d_recs, d_reps, q_lo, n_q, k, d_head, nodes_cap, d_edges, edges_cap, loops, d_workspace, d_loops, d_rep,
                                stream=None):
        """lsd_enqueue_pg_loops_device on raw device addresses: the distinct loops (d_loops: PG_LOOP_REC_DTYPE [max_loops]; d_rep: one
        PG_LOOPS_REP_DTYPE) among the records enqueue_pg_recognize_all_device left for (q_lo, n_q, k), pairs near a closure edge of the
        graph left out.  loops: pg_loops(); d_workspace: pg_loops_workspace_bytes(n_q, k, edges_cap) bytes.  Asynchronous."""
        return self._chk(self.L.lsd_enqueue_pg_loops_device(self.h, d_recs, d_reps, int(q_lo), int(n_q), int(k), d_head, int(nodes_cap), d_edges,
                                                            int(edges_cap), pg_loops(loops), d_workspace, d_loops, d_rep, stream))

    def enqueue_pg_loop_select_device(self, d_head, d_nodes, nodes_cap, d_store, d_store_lens, store_stride, gap, window, d_loops, d_loops_rep, m,
                                      d_near, d_sel, d_q_scan, d_q_len, d_q_pose, stream=None):
        """lsd_enqueue_pg_loop_select_device on raw device addresses: what enqueue_pg_recognize_device leaves -- near record, selection, the
        gathered query, the anchor's pose turned by the shift -- for loop m of enqueue_pg_loops_device's records.  Asynchronous."""
        return self._chk(self.L.lsd_enqueue_pg_loop_select_device(self.h, d_head, d_nodes, int(nodes_cap), d_store, d_store_lens, int(store_stride),
                                                                  int(gap), int(window), d_loops, d_loops_rep, int(m), d_near, d_sel, d_q_scan,
                                                                  d_q_len, d_q_pose, stream))

    def pg_recognize_all(self, desc, q_lo=0, n_q=None, place=None):
        """lsd_pg_recognize_all from host arrays: desc PG_DESC_DTYPE [n] and the queries q_lo .. q_lo + n_q - 1 (n_q None: up to n) ->
        (records PG_PLACE_REC_DTYPE [n_q, k], reports PG_PLACE_REP_DTYPE [n_q]).  place: pg_place().  Blocking."""
        de, par = np.ascontiguousarray(desc, PG_DESC_DTYPE).reshape(-1), pg_place(place)
        nq = len(de) - int(q_lo) if n_q is None else int(n_q)
        recs, reps = np.zeros((max(nq, 0), max(par.k, 0)), PG_PLACE_REC_DTYPE), np.zeros(max(nq, 0), PG_PLACE_REP_DTYPE)
        self._chk(self.L.lsd_pg_recognize_all(self.h, de.ctypes.data if len(de) else None, len(de), int(q_lo), nq, par, recs.ctypes.data,
                                              reps.ctypes.data))
        return recs, reps

    def pg_loops(self, recs, reps, edges, loops=None):
        """lsd_pg_loops from host arrays: recs PG_PLACE_REC_DTYPE [n_q, k] and reps PG_PLACE_REP_DTYPE [n_q] as pg_recognize_all returns
        them, the graph's edges PG_EDGE_DTYPE [m] -> (loops PG_LOOP_REC_DTYPE [max_loops], report PG_LOOPS_REP_DTYPE).  loops:
        pg_loops().  Blocking."""
        rp = np.ascontiguousarray(reps, PG_PLACE_REP_DTYPE).reshape(-1)
        rc = np.ascontiguousarray(recs, PG_PLACE_REC_DTYPE)
        k = rc.shape[-1] if rc.ndim == 2 else (rc.size // len(rp) if len(rp) else 1)
        rc, ed, par = rc.reshape(-1), np.ascontiguousarray(edges, PG_EDGE_DTYPE).reshape(-1), pg_loops(loops)
        if len(rc) != len(rp) * k:
            raise LsdError(LSD_ERR_INVALID, "recs must be [n_q, k] with one report per query")
        out, rep = np.zeros(min(max(par.max_loops, 1), PG_LOOPS_MAX), PG_LOOP_REC_DTYPE), np.zeros(1, PG_LOOPS_REP_DTYPE)
        self._chk(self.L.lsd_pg_loops(self.h, rc.ctypes.data if len(rc) else None, rp.ctypes.data if len(rp) else None, len(rp), int(k),
                                      ed.ctypes.data if len(ed) else None, len(ed), par, out.ctypes.data, rep.ctypes.data))
        return out, rep[0]

    def enqueue_pg_reduce_device(self, d_head, d_nodes, nodes_cap, d_edges, edges_cap, d_tracks, n_tracks, d_store, d_store_lens, store_stride,
                                 d_desc, reduce, d_map, d_rep, d_workspace, stream=None):
        """lsd_enqueue_pg_reduce_device on raw device addresses: the keyframes of a place that `keep` older ones already hold are
        retired where the odometry chain can be contracted across them, and nodes, edges, ALL n_tracks track records, store rows,
        lengths and descriptors (d_desc may be None) are compacted in place.  d_map: int32 [nodes_cap], the new index of every node or
        -1; d_rep: one PG_REDUCE_REP_DTYPE or None; d_workspace: pg_reduce_workspace_bytes(nodes_cap, edges_cap, store_stride) bytes.
        reduce: pg_reduce().  Asynchronous."""
        return self._chk(self.L.lsd_enqueue_pg_reduce_device(self.h, d_head, d_nodes, int(nodes_cap), d_edges, int(edges_cap), d_tracks, int(n_tracks),
                                                             d_store, d_store_lens, int(store_stride), d_desc, pg_reduce(reduce), d_map, d_rep,
                                                             d_workspace, stream))

    def pg_reduce(self, head, nodes, edges, tracks, store, store_lens, desc=None, reduce=None):
        """lsd_pg_reduce from host arrays: the graph head (PG_HEAD_DTYPE), nodes [nodes_cap], edges [edges_cap], tracks (PG_TRACK_DTYPE
        [n_tracks]), store float64 [nodes_cap, store_stride, 2], store_lens int32 [nodes_cap] and desc (PG_DESC_DTYPE [nodes_cap], or
        None).  Returns (head, nodes, edges, tracks, store, store_lens, desc, map int32 [nodes_cap], report): new arrays.  reduce:
        pg_reduce().  Blocking."""
        hd, no, ed = np.array(head, PG_HEAD_DTYPE).reshape(1), np.array(nodes, PG_NODE_DTYPE).reshape(-1), np.array(edges, PG_EDGE_DTYPE).reshape(-1)
        tr, st, sl = np.array(tracks, PG_TRACK_DTYPE).reshape(-1), np.array(store, np.float64), np.array(store_lens, np.int32).reshape(-1)
        de = None if desc is None else np.array(desc, PG_DESC_DTYPE).reshape(-1)
        if st.ndim != 3 or st.shape[0] != len(no) or st.shape[2] != 2 or len(sl) != len(no) or (de is not None and len(de) != len(no)):
            raise LsdError(LSD_ERR_INVALID, "store [nodes_cap, store_stride, 2], store_lens [nodes_cap], desc [nodes_cap] or None")
        mp, rep = np.zeros(len(no), np.int32), np.zeros(1, PG_REDUCE_REP_DTYPE)
        self._chk(self.L.lsd_pg_reduce(self.h, hd.ctypes.data, no.ctypes.data, len(no), ed.ctypes.data, len(ed), tr.ctypes.data, len(tr), st.ctypes.data,
                                       sl.ctypes.data, st.shape[1], None if de is None else de.ctypes.data, pg_reduce(reduce), mp.ctypes.data,
                                       rep.ctypes.data))
        return hd[0], no, ed, tr, st, sl, de, mp, rep[0]

    def enqueue_map_update_device(self, d_grid, cols, rows, res, z_occ_max_dis, d_map, d_map_cache, d_lines, max_lines, d_count,
                                  d_line_im=None, params=None, stream=None):
        """lsd_enqueue_map_update_device: the map callback (cells -> map -> mapCache -> LSD with the map rewritten) as one enqueue on
        raw device addresses; asynchronous."""
        p = params or make_params()
        return self._chk(self.L.lsd_enqueue_map_update_device(self.h, d_grid, cols, rows, float(res), float(z_occ_max_dis), C.byref(p), d_map,
                                                              d_map_cache, d_lines, max_lines, d_count, d_line_im, stream))

    def reserve_map_update(self, cols, rows):
        """lsd_reserve_map_update: after it enqueue_map_update_device of a cols x rows grid (or a smaller one) never allocates or waits."""
        self._chk(self.L.lsd_reserve_map_update(self.h, cols, rows))

    def occupancy_to_map(self, grid_i8):
        """lsd_occupancy_to_map on an int8 [rows, cols] OccupancyGrid; returns the uint8 map."""
        assert grid_i8.dtype == np.int8 and grid_i8.ndim == 2 and grid_i8.flags.c_contiguous
        rows, cols = grid_i8.shape
        out = np.zeros((rows, cols), np.uint8)
        self._chk(self.L.lsd_occupancy_to_map(self.h, grid_i8.ctypes.data, cols, rows, out.ctypes.data, out.strides[0]))
        return out

    def enqueue_occupancy_to_map_device(self, d_grid, n_cells, d_map, stream=None):
        return self._chk(self.L.lsd_enqueue_occupancy_to_map_device(self.h, d_grid, n_cells, d_map, stream))

    # -- mapping with known poses -------------------------------------------------------------------
    def enqueue_grid_integrate_device(self, d_scans, d_lens, n_scans, stride, d_poses, pose_pitch, map_param, range_max, d_pass, d_hit,
                                      stream=None):
        """lsd_enqueue_grid_integrate_device on device addresses: n_scans ingested scans (d_scans at a pitch of `stride` readings, d_lens),
        scan i at the pose in the first three doubles of the record at d_poses + i * pose_pitch bytes (24: packed poses, 720: lsd_fa_state,
        768: lsd_fa_carry), counted into the uint32 planes d_pass / d_hit of map_param's grid; asynchronous."""
        return self._chk(self.L.lsd_enqueue_grid_integrate_device(self.h, d_scans, d_lens, int(n_scans), int(stride), d_poses, int(pose_pitch),
                                                                  _map_param(map_param), float(range_max), d_pass, d_hit, stream))

    def enqueue_grid_publish_device(self, d_pass, d_hit, n_cells, d_grid, min_pass=2, occ_num=1, occ_den=10, stream=None):
        """lsd_enqueue_grid_publish_device on device addresses: d_grid[i] = -1 where d_pass[i] < min_pass, else 100 where
        d_hit[i] * occ_den >= d_pass[i] * occ_num, else 0; asynchronous."""
        n_cells, min_pass, occ_num, occ_den = _u32s(n_cells, min_pass, occ_num, occ_den, limit=(1 << 64, 1 << 32, 1 << 32, 1 << 32))
        return self._chk(self.L.lsd_enqueue_grid_publish_device(self.h, d_pass, d_hit, n_cells, min_pass, occ_num, occ_den, d_grid, stream))

    def grid_integrate(self, scans, lens, poses, map_param, range_max, pass_counts=None, hit_counts=None):
        """lsd_grid_integrate from host arrays: scans float64 [n, stride, 2], lens int32 [n], poses float64 [n, 3] (x, y in map pixels, ang
        in degrees), the planes uint32 [rows, cols] (None: zeros).  Returns (pass, hit): new arrays, the given counts plus this call's."""
        sc, ln, po, ok = _host_scans(scans, lens, poses)
        mp = _map_param(map_param)
        if not ok or mp.oriMapCol <= 0 or mp.oriMapRow <= 0:
            raise LsdError(LSD_ERR_INVALID, "scans [n, stride, 2], lens [n], poses [n, 3], a grid of at least one cell")
        shape = (mp.oriMapRow, mp.oriMapCol)
        planes = []
        for a in (pass_counts, hit_counts):
            a = np.zeros(shape, np.uint32) if a is None else np.array(a, np.uint32).reshape(shape)
            planes.append(np.ascontiguousarray(a))
        self._chk(self.L.lsd_grid_integrate(self.h, sc.ctypes.data, ln.ctypes.data, len(ln), max(sc.shape[1], 0), po.ctypes.data, mp,
                                            float(range_max), planes[0].ctypes.data, planes[1].ctypes.data))
        return planes[0], planes[1]

    # -- ray casting on the grid (k_gridray.hip) -------------------------------------
    def enqueue_grid_raycast_device(self, d_scans, d_lens, n_scans, stride, d_poses, pose_pitch, map_param, range_max, d_grid, ray, d_out,
                                    d_sum, d_scans_out=None, stream=None):
        """lsd_enqueue_grid_raycast_device on device addresses: scans, lengths and poses as enqueue_grid_integrate_device reads them, cast
        through the int8 grid d_grid (rows x cols of map_param); ray: an lsd_grid_ray_par or what grid_ray() takes (its tol must be
        given: no mapper is known here).  d_out receives n_scans x stride records of 32 bytes (GRID_RAY_DTYPE; those at i < len),
        d_sum n_scans records of 64 bytes (GRID_RAY_SUM_DTYPE), which are a d_poses argument of pitch 64 themselves; d_scans_out (or
        None; d_scans itself is allowed) the screened scans.  Asynchronous."""
        return self._chk(self.L.lsd_enqueue_grid_raycast_device(self.h, d_scans, d_lens, int(n_scans), int(stride), d_poses, int(pose_pitch),
                                                                _map_param(map_param), float(range_max), d_grid, grid_ray(ray), d_out, d_sum,
                                                                d_scans_out, stream))

    def grid_raycast(self, scans, lens, poses, map_param, range_max, grid, ray, out=None, sums=None, scans_out=None):
        """lsd_grid_raycast from host arrays: scans float64 [n, stride, 2], lens int32 [n], poses float64 [n, 3], grid int8 [rows, cols].
        Returns (records GRID_RAY_DTYPE [n, stride], summaries GRID_RAY_SUM_DTYPE [n], screened scans float64 [n, stride, 2]): new
        arrays that start from out / sums / scans_out where given (zeros otherwise) -- only the slots at i < len are written.  Blocking."""
        sc, ln, po, ok = _host_scans(scans, lens, poses)
        mp = _map_param(map_param)
        gr = np.ascontiguousarray(grid, np.int8)
        if not ok or gr.shape != (mp.oriMapRow, mp.oriMapCol):
            raise LsdError(LSD_ERR_INVALID, "scans [n, stride, 2], lens [n], poses [n, 3], grid int8 [rows, cols]")
        n, stride = sc.shape[:2]
        o = np.zeros((n, stride), GRID_RAY_DTYPE) if out is None else np.array(out, GRID_RAY_DTYPE).reshape(n, stride)
        su = np.zeros(n, GRID_RAY_SUM_DTYPE) if sums is None else np.array(sums, GRID_RAY_SUM_DTYPE).reshape(n)
        so = np.zeros((n, stride, 2)) if scans_out is None else np.array(scans_out, np.float64).reshape(n, stride, 2)
        self._chk(self.L.lsd_grid_raycast(self.h, sc.ctypes.data, ln.ctypes.data, n, max(stride, 0), po.ctypes.data, mp, float(range_max),
                                          gr.ctypes.data, grid_ray(ray), o.ctypes.data, su.ctypes.data, so.ctypes.data))
        return o, su, so

    # -- correlative scan-to-grid matching ----------------------------------------------------------
    def enqueue_grid_likelihood_device(self, d_pass, d_hit, cols, rows, d_corr, min_pass=2, occ_num=1, occ_den=10, smear=None, stream=None):
        """lsd_enqueue_grid_likelihood_device on device addresses: d_corr[y][x] (uint8, rows x cols) = the largest smear.w[|v|][|u|] over the
        occupied cells (x + u, y + v) within smear.radius (occupied: what the publish rule gives 100), 0 if none; asynchronous.  smear: an
        lsd_grid_smear or what grid_smear() takes (None: grid_smear_default(1.0, 3))."""
        min_pass, occ_num, occ_den = _u32s(min_pass, occ_num, occ_den, limit=(1 << 32,) * 3)
        return self._chk(self.L.lsd_enqueue_grid_likelihood_device(self.h, d_pass, d_hit, int(cols), int(rows), min_pass, occ_num, occ_den,
                                                                   grid_smear(smear), d_corr, stream))

    def enqueue_grid_match_device(self, d_scans, d_lens, n_scans, stride, d_poses, pose_pitch, map_param, range_max, d_corr, search, d_out,
                                  stream=None):
        """lsd_enqueue_grid_match_device on device addresses: scans, lengths and poses as enqueue_grid_integrate_device reads them, matched on
        the plane d_corr over the window `search` (an lsd_grid_search or what grid_search() takes); d_out receives n_scans records of 56
        bytes (GRID_MATCH_DTYPE), which are a d_poses argument of pitch 56 themselves; asynchronous."""
        return self._chk(self.L.lsd_enqueue_grid_match_device(self.h, d_scans, d_lens, int(n_scans), int(stride), d_poses, int(pose_pitch),
                                                              _map_param(map_param), float(range_max), d_corr, grid_search(search), d_out, stream))

    def grid_match(self, scans, lens, poses, map_param, range_max, corr, search):
        """lsd_grid_match from host arrays: scans float64 [n, stride, 2], lens int32 [n], poses float64 [n, 3], corr uint8 [rows, cols].
        Returns the n records as a numpy array of GRID_MATCH_DTYPE.  Blocking."""
        sc, ln, po, ok = _host_scans(scans, lens, poses)
        mp = _map_param(map_param)
        co = np.ascontiguousarray(corr, np.uint8)
        if not ok or co.shape != (mp.oriMapRow, mp.oriMapCol):
            raise LsdError(LSD_ERR_INVALID, "scans [n, stride, 2], lens [n], poses [n, 3], corr uint8 [rows, cols]")
        out = np.zeros(len(ln), GRID_MATCH_DTYPE)
        self._chk(self.L.lsd_grid_match(self.h, sc.ctypes.data, ln.ctypes.data, len(ln), max(sc.shape[1], 0), po.ctypes.data, mp, float(range_max),
                                        co.ctypes.data, grid_search(search), out.ctypes.data))
        return out

    # -- the same match, coarse to fine (k_gridmatch_mr.hip) -------------------------
    def enqueue_grid_coarse_device(self, d_corr, cols, rows, block, d_coarse, stream=None):
        """lsd_enqueue_grid_coarse_device on device addresses: d_coarse (uint8, (rows + block - 1) x (cols + block - 1)) = the maximum of
        d_corr over the block x block cells from (x - block + 1, y - block + 1) up, cells outside the grid as 0; asynchronous."""
        return self._chk(self.L.lsd_enqueue_grid_coarse_device(self.h, d_corr, int(cols), int(rows), int(block), d_coarse, stream))

    def enqueue_grid_match_mr_device(self, d_scans, d_lens, n_scans, stride, d_poses, pose_pitch, map_param, range_max, d_corr, d_coarse, block,
                                     search, d_out, d_stats=None, stream=None):
        """lsd_enqueue_grid_match_mr_device on device addresses: enqueue_grid_match_device's records, found by a coarse-to-fine search over
        blocks of block x block translations; d_coarse is what enqueue_grid_coarse_device made of d_corr with the same block; d_stats (or
        None) receives n_scans records of 16 bytes (GRID_MATCH_MR_STATS_DTYPE); asynchronous."""
        return self._chk(self.L.lsd_enqueue_grid_match_mr_device(self.h, d_scans, d_lens, int(n_scans), int(stride), d_poses, int(pose_pitch),
                                                                 _map_param(map_param), float(range_max), d_corr, d_coarse, int(block),
                                                                 grid_search(search), d_out, d_stats, stream))

    def grid_match_mr(self, scans, lens, poses, map_param, range_max, corr, block, search, stats=False):
        """lsd_grid_match_mr from host arrays (those of grid_match): the n records, and with stats=True (records, the n statistics records as
        a numpy array of GRID_MATCH_MR_STATS_DTYPE).  Blocking."""
        sc, ln, po, ok = _host_scans(scans, lens, poses)
        mp = _map_param(map_param)
        co = np.ascontiguousarray(corr, np.uint8)
        if not ok or co.shape != (mp.oriMapRow, mp.oriMapCol):
            raise LsdError(LSD_ERR_INVALID, "scans [n, stride, 2], lens [n], poses [n, 3], corr uint8 [rows, cols]")
        out = np.zeros(len(ln), GRID_MATCH_DTYPE)
        st = np.zeros(len(ln), GRID_MATCH_MR_STATS_DTYPE)
        self._chk(self.L.lsd_grid_match_mr(self.h, sc.ctypes.data, ln.ctypes.data, len(ln), max(sc.shape[1], 0), po.ctypes.data, mp,
                                           float(range_max), co.ctypes.data, int(block), grid_search(search), out.ctypes.data,
                                           st.ctypes.data if stats else None))
        return (out, st) if stats else out

    # -- global scan-to-grid localisation (k_gridlocate.hip) -------------------------
    def enqueue_grid_pyramid_device(self, d_corr, cols, rows, levels, d_pyramid, stream=None):
        """lsd_enqueue_grid_pyramid_device on device addresses: d_pyramid (uint8, grid_pyramid_bytes(cols, rows, levels) bytes) = the
        planes 0..levels of block maxima of d_corr one behind the other (level h at grid_pyramid_offset(cols, rows, h)); asynchronous."""
        return self._chk(self.L.lsd_enqueue_grid_pyramid_device(self.h, d_corr, int(cols), int(rows), int(levels), d_pyramid, stream))

    def enqueue_grid_locate_device(self, d_scans, d_lens, n_scans, stride, map_param, range_max, d_pyramid, locate, d_out, d_stats=None,
                                   stream=None):
        """lsd_enqueue_grid_locate_device on device addresses: scans and lengths as enqueue_grid_integrate_device reads them, located
        without a prior in the box and the headings `locate` names (an lsd_grid_locate_par or what grid_locate() takes) on the pyramid
        enqueue_grid_pyramid_device made of the lookup plane; d_out receives n_scans records of 64 bytes (GRID_LOCATE_DTYPE), which are a
        d_poses argument of pitch 64 themselves; d_stats (or None) n_scans records of 48 bytes (GRID_LOCATE_STATS_DTYPE); asynchronous."""
        mp = _map_param(map_param)
        return self._chk(self.L.lsd_enqueue_grid_locate_device(self.h, d_scans, d_lens, int(n_scans), int(stride), mp, float(range_max), d_pyramid,
                                                               grid_locate(locate, cols=mp.oriMapCol, rows=mp.oriMapRow), d_out, d_stats, stream))

    def grid_locate(self, scans, lens, map_param, range_max, corr, locate=None, stats=False):
        """lsd_grid_locate from host arrays: scans float64 [n, stride, 2], lens int32 [n], corr uint8 [rows, cols].  Returns the n records as
        a numpy array of GRID_LOCATE_DTYPE, and with stats=True (records, the n statistics records as GRID_LOCATE_STATS_DTYPE).  Blocking."""
        sc, ln, _, ok = _host_scans(scans, lens, np.zeros((len(np.atleast_1d(lens)), 3)))
        mp = _map_param(map_param)
        co = np.ascontiguousarray(corr, np.uint8)
        if not ok or co.shape != (mp.oriMapRow, mp.oriMapCol):
            raise LsdError(LSD_ERR_INVALID, "scans [n, stride, 2], lens [n], corr uint8 [rows, cols]")
        out = np.zeros(len(ln), GRID_LOCATE_DTYPE)
        st = np.zeros(len(ln), GRID_LOCATE_STATS_DTYPE)
        self._chk(self.L.lsd_grid_locate(self.h, sc.ctypes.data, ln.ctypes.data, len(ln), max(sc.shape[1], 0), mp, float(range_max), co.ctypes.data,
                                         grid_locate(locate, cols=mp.oriMapCol, rows=mp.oriMapRow), out.ctypes.data,
                                         st.ctypes.data if stats else None))
        return (out, st) if stats else out

    def enqueue_grid_locate_tight_device(self, d_scans, d_lens, n_scans, stride, map_param, range_max, d_pyramid, locate, tight, d_out,
                                         d_stats=None, stream=None):
        """lsd_enqueue_grid_locate_tight_device on device addresses: enqueue_grid_locate_device with the bound raised level by level
        (DESIGN.md 8.1.14); tight: what grid_locate_tight() takes, 0 included; d_stats (or None) receives n_scans records of 128 bytes
        (GRID_LOCATE_TIGHT_STATS_DTYPE); asynchronous."""
        mp = _map_param(map_param)
        return self._chk(self.L.lsd_enqueue_grid_locate_tight_device(self.h, d_scans, d_lens, int(n_scans), int(stride), mp, float(range_max),
                                                                     d_pyramid, grid_locate(locate, cols=mp.oriMapCol, rows=mp.oriMapRow),
                                                                     grid_locate_tight(tight), d_out, d_stats, stream))

    def grid_locate_tight(self, scans, lens, map_param, range_max, corr, locate=None, tight=True, stats=False):
        """lsd_grid_locate_tight from host arrays: grid_locate under the tight rule (tight: what grid_locate_tight() takes; the entry is
        taken with 0 as well); with stats=True the statistics are GRID_LOCATE_TIGHT_STATS_DTYPE.  Blocking."""
        sc, ln, _, ok = _host_scans(scans, lens, np.zeros((len(np.atleast_1d(lens)), 3)))
        mp = _map_param(map_param)
        co = np.ascontiguousarray(corr, np.uint8)
        if not ok or co.shape != (mp.oriMapRow, mp.oriMapCol):
            raise LsdError(LSD_ERR_INVALID, "scans [n, stride, 2], lens [n], corr uint8 [rows, cols]")
        out = np.zeros(len(ln), GRID_LOCATE_DTYPE)
        st = np.zeros(len(ln), GRID_LOCATE_TIGHT_STATS_DTYPE)
        self._chk(self.L.lsd_grid_locate_tight(self.h, sc.ctypes.data, ln.ctypes.data, len(ln), max(sc.shape[1], 0), mp, float(range_max),
                                               co.ctypes.data, grid_locate(locate, cols=mp.oriMapCol, rows=mp.oriMapRow), grid_locate_tight(tight),
                                               out.ctypes.data, st.ctypes.data if stats else None))
        return (out, st) if stats else out

    # -- the response around a match (k_gridresponse.hip) -----------------------------
    def enqueue_grid_response_device(self, d_scans, d_lens, n_scans, stride, d_poses, pose_pitch, d_records, map_param, range_max, d_corr,
                                     ang_step, response, d_out, d_volume=None, stream=None):
        """lsd_enqueue_grid_response_device on device addresses: the scans, lengths and ORIGINAL poses a match entry was given, and the
        n_scans records (56 bytes each) it wrote; ang_step is the search's; response: an lsd_grid_response or what grid_response() takes.
        d_out receives n_scans records of 192 bytes (GRID_RESPONSE_DTYPE), which are a d_poses argument of pitch 192 themselves; d_volume
        (or None) the n_scans x (2 ra + 1)(2 ry + 1)(2 rx + 1) uint32 scores; asynchronous."""
        return self._chk(self.L.lsd_enqueue_grid_response_device(self.h, d_scans, d_lens, int(n_scans), int(stride), d_poses, int(pose_pitch),
                                                                 d_records, _map_param(map_param), float(range_max), d_corr, float(ang_step),
                                                                 grid_response(response), d_out, d_volume, stream))

    def grid_response(self, scans, lens, poses, records, map_param, range_max, corr, ang_step, response=None, volume=False):
        """lsd_grid_response from host arrays (those of grid_match, and its records as a numpy array of GRID_MATCH_DTYPE): the n response
        records as a numpy array of GRID_RESPONSE_DTYPE, and with volume=True (records, the scores: uint32 [n, 2 ra + 1, 2 ry + 1,
        2 rx + 1]).  Blocking."""
        sc, ln, po, ok = _host_scans(scans, lens, poses)
        rec = np.ascontiguousarray(records)
        mp = _map_param(map_param)
        co = np.ascontiguousarray(corr, np.uint8)
        if not ok or co.shape != (mp.oriMapRow, mp.oriMapCol) or rec.dtype != GRID_MATCH_DTYPE or rec.shape != (len(ln),):
            raise LsdError(LSD_ERR_INVALID, "scans [n, stride, 2], lens [n], poses [n, 3], records GRID_MATCH_DTYPE [n], corr uint8 [rows, cols]")
        rp = grid_response(response)
        out = np.zeros(len(ln), GRID_RESPONSE_DTYPE)
        vol = np.zeros((len(ln), 2 * rp.ra + 1, 2 * rp.ry + 1, 2 * rp.rx + 1) if volume else (0,), np.uint32)
        self._chk(self.L.lsd_grid_response(self.h, sc.ctypes.data, ln.ctypes.data, len(ln), max(sc.shape[1], 0), po.ctypes.data, rec.ctypes.data,
                                           mp, float(range_max), co.ctypes.data, float(ang_step), rp, out.ctypes.data,
                                           vol.ctypes.data if volume else None))
        return (out, vol) if volume else out

    def reserve(self, n, cols, rows):
        self._chk(self.L.lsd_reserve(self.h, n, cols, rows))

    def synchronize(self):
        self._chk(self.L.lsd_synchronize(self.h))

    def fetch_stats_block(self, n):
        """The raw counter records (the values of fetch(i, DBG_STATS, ...), in its order) of the first n images of the last
        batch as an (n, 48) int64 array, in one copy (developer probes)."""
        a = np.zeros((n, 48), np.int64)
        self._chk(self.L.lsd_debug_fetch(self.h, 0, DBG_STATS, a.ctypes.data, a.nbytes))
        return a

    def last_region_cycles(self, n):
        """lsd_last_region_cycles: shader clocks of the region stage per image of the last batch (the cost shard_balanced deals by)."""
        a = np.zeros(n, np.int64)
        self._chk(self.L.lsd_last_region_cycles(self.h, n, a.ctypes.data))
        return a

    def last_sensitivity(self, n):
        """lsd_last_sensitivity: per image of the last batch, the number of decisions taken within the noise of the reference's libm
        (0: the image's result is the reference's under any libm within one ulp of correct rounding)."""
        a = np.zeros(n, np.int32)
        self._chk(self.L.lsd_last_sensitivity(self.h, n, a.ctypes.data))
        return a

    def timings(self):
        ms = (C.c_float * 6)()
        self._chk(self.L.lsd_last_timings(self.h, ms))
        return dict(zip(("gauss", "gradient", "sort", "region", "lines", "total"), [float(x) for x in ms]))

    # -- introspection ----------------------------------------------------------------------------
    def set_stop_after(self, stage):
        self._chk(self.L.lsd_set_stop_after(self.h, stage))

    def set_trace(self, on):
        self._chk(self.L.lsd_set_trace(self.h, 1 if on else 0))

    def set_fused_front(self, on):
        """lsd_set_fused_front: Gaussian and gradient pass as one kernel where that applies (default on; results are identical)."""
        self._chk(self.L.lsd_set_fused_front(self.h, 1 if on else 0))

    def set_fused_lines(self, on):
        """lsd_set_fused_lines: the region stage writes an image's lines when it has finished it, no kernel behind the batch (default on; results are identical)."""
        self._chk(self.L.lsd_set_fused_lines(self.h, 1 if on else 0))

    def set_host_max_lines(self, max_lines):
        """Line capacity per image of run / run_batch (default HOST_MAX_LINES_DEFAULT); more lines -> LsdError(LSD_ERR_CAPACITY)."""
        self._chk(self.L.lsd_set_host_max_lines(self.h, max_lines))

    def set_cost_history(self, on):
        """lsd_set_cost_history: start the images of a batch in the order of their cost in this context's previous call (same maps from call to call)."""
        self._chk(self.L.lsd_set_cost_history(self.h, 1 if on else 0))

    def debug_set_tuning(self, name, value):
        """Test / developer hook (lsd_debug_set_tuning): a schedule setting of the region stage by name; no result depends on any."""
        self._chk(self.L.lsd_debug_set_tuning(self.h, name.encode(), int(value)))

    def debug_set_stamp_budget(self, grows):
        """Test hook (lsd_debug_set_stamp_budget): curMap stamp ids per wavefront and run before the stamps are cleared."""
        self._chk(self.L.lsd_debug_set_stamp_budget(self.h, grows))

    def debug_poison_front(self):
        """Test hook (lsd_debug_poison_front): 0xFF bytes into every array the front end fills, so that the next call's omissions show."""
        self._chk(self.L.lsd_debug_poison_front(self.h))

    def set_region_waves(self, waves):
        """0: automatic, 4 / 8: force the region-stage variant (results are identical)."""
        self._chk(self.L.lsd_set_region_waves(self.h, waves))

    def set_region_help(self, waves):
        """Helper wavefronts per image of the region stage's help across workgroups (lsd_set_region_help): 0 switches it off (the
        setting for several batches in flight on several contexts), -1 restores the default.  Results are identical."""
        self._chk(self.L.lsd_set_region_help(self.h, waves))

    def fetch(self, image, what, shape_wh):
        """Returns the intermediate `what` (DBG_*) of image `image` of the last run as a numpy array."""
        w, h = shape_wh
        npx = w * h

        def get(kind, dtype, count):
            a = np.zeros(max(count, 1), dtype)
            self._chk(self.L.lsd_debug_fetch(self.h, image, kind, a.ctypes.data, a.nbytes))
            return a[:count]

        if what in (DBG_GAUSS, DBG_MAG, DBG_DEG):
            return get(what, np.float64, npx).reshape(h, w)
        if what == DBG_STATE:
            return get(what, np.uint32, npx).reshape(h, w)
        if what == DBG_PW:                               # the packed pixel word: fp32 angle & ~3 | code (STATE: its usedMap value)
            return get(what, np.uint32, npx).reshape(h, w)
        if what == DBG_SINCOS:                           # [..., 0] sin, [..., 1] cos; defined only where the pixel's code is 0
            return get(what, np.float64, 2 * npx).reshape(h, w, 2)
        if what in (DBG_NB, DBG_GRAD_TIES):
            return int(get(what, np.int32, 1)[0])
        if what == DBG_NSEED:
            return int(get(what, np.int32, 1)[0])
        if what == DBG_MAXGRAD:
            return float(get(what, np.float64, 1)[0])
        if what == DBG_ORDER:
            return get(what, np.uint32, npx)[:self.fetch(image, DBG_NB, shape_wh)]
        if what == DBG_ORDER_VAL:
            return get(what, np.uint16, npx)[:self.fetch(image, DBG_NB, shape_wh)]
        if what == DBG_STATS:
            v = get(what, np.int64, 48)
            d = dict(zip(("grow_calls", "grown_px", "nfa_calls", "rrr_calls", "rrr_passes", "rrr_sentinel_drops",
                          "rrr_oob_reads", "cycles_refill", "cycles_total", "cycles_grow", "cycles_rect",
                          "cycles_nfa", "cycles_mark", "small_bails", "wait_noslot", "seeds", "exact_angle_evals",
                          "tile_fetches", "batches", "cycles_tiles", "spec_redos", "spec_discards", "cycles_wait", "small_steps",
                          "refill_rounds", "cycles_eval", "cycles_sums", "cycles_refine", "cycles_small", "cycles_select", "cycles_commit",
                          "wait_noseed", "requeued_ahead", "cycles_eval_at_cursor", "depth_end", "nfa_min_abs_enc", "nfa_min_gap_enc", "help_exports", "help_evals", "near_ties",
                          "wd_commit", "wd_next", "wd_nseeds", "wd_state", "wd_nbig", "wd_lock", "wd_pend", "wd_wave"),
                         [int(x) for x in v]))
            d["set_answers"], d["sets_founded"] = int(v[41]), int(v[42])   # evaluations answered by a certified uniform set / sets founded (region/eval.h)
            d["cycles_nfa_count"], d["nfa_tail_iters"] = int(v[43]), int(v[44])   # developer build: cycles of the NFA's pixel count, iterations of its tail sum
            d["grow_any_calls"] = int(v[45]) >> 8   # RegionGrower calls that took the any-tolerance function (region/grow.h: grow_any; tolerances of 1.5 rad and more, NaN); bits 3..0 of the word: the image's XCC
            d["nfa_bracket_misses"] = int(v[40])   # stopping tests of the NFA's tail left to the correctly rounded pow / log10 (an image the watchdog gave up keeps its record here instead)
            # how close RectangleImprover's comparisons came to a tie, as margins (distance of the operands over what an ulp of exp / log10 /
            # pow can move them; region/nfa.h: improve()): smallest for a logNFA compared with 0, smallest for two compared NFA values (inf: none seen)
            for k in ("nfa_min_abs", "nfa_min_gap"):
                enc = d.pop(k + "_enc")
                d[k] = float("inf") if enc == 0 else float(np.array([0x7ff0000000000000 - enc], np.uint64).view(np.float64)[0])
            return d
        if what == DBG_SEEDS:
            ns = self.fetch(image, DBG_NSEED, shape_wh)
            return get(what, SEED_DTYPE, ns)
        raise ValueError(what)

    def eval_math(self, fn, a, b=None):
        """Device sin/cos (fn 0), atan2(a, b) (fn 1), atan (fn 2) of float64 arrays, or the region stage's fp32 estimate of
        sin/cos of the packed angle (fn 3) (test hook)."""
        a = np.ascontiguousarray(a, np.float64)
        b = None if b is None else np.ascontiguousarray(b, np.float64)
        o0, o1 = np.zeros_like(a), np.zeros_like(a)
        self._chk(self.L.lsd_debug_eval_math(self.h, fn, a.ctypes.data, None if b is None else b.ctypes.data,
                                             o0.ctypes.data, o1.ctypes.data, a.size))
        return o0, o1

    def debug_lines(self, recs, rows, cols, want_lineim=True):
        """lsd_debug_lines: K5 alone on rectangles float64 [n, 4] = (x1, y1, x2, y2) in the cells of a rows x cols map -> (records
        LINE_DTYPE [n], lineIm or None) (test hook)."""
        r = np.ascontiguousarray(recs, np.float64).reshape(-1, 4)
        lines = np.zeros(len(r), LINE_DTYPE)
        im = np.zeros((rows, cols), np.uint8) if want_lineim else None
        self._chk(self.L.lsd_debug_lines(self.h, r.ctypes.data, len(r), cols, rows, lines.ctypes.data, im.ctypes.data if want_lineim else None))
        return lines, im

    def fetch_recs(self, image, count):
        a = np.zeros(max(count * 12, 1), np.float64)
        self._chk(self.L.lsd_debug_fetch(self.h, image, DBG_RECS, a.ctypes.data, a.nbytes))
        return a[:count * 12].reshape(count, 12)


# ---- the reference's own names (LSD/myLSD.h:123-132) ----------------------------------------------
class structLSD:
    """structLSD (LSD/myLSD.h:123-127): lineIm (CV_8UC1 rows x cols, 0/255), linesInfo, len_linesInfo."""

    def __init__(self, lineIm, linesInfo):
        self.lineIm = lineIm
        self.linesInfo = linesInfo
        self.len_linesInfo = len(linesInfo)


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


def myLineSegmentDetector(MapGray, oriMapCol, oriMapRow, sca, sig, angThre, denThre, pseBin, ctx=None):
    """mylsd::myLineSegmentDetector (LSD/myLSD.h:132, LSD/myLSD.cpp:129): same argument meaning, same
    in-place rewrite of MapGray, returns structLSD.  No validation beyond the C ABI's, like the reference."""
    if MapGray.shape != (oriMapRow, oriMapCol):
        raise LsdError(LSD_ERR_INVALID, "MapGray must be oriMapRow x oriMapCol")
    ctx = ctx or default_context()
    lines, line_im = ctx.run(MapGray, make_params(sca, sig, angThre, denThre, pseBin))
    return structLSD(line_im, lines)


def createMapCache(MapGray, res, ctx=None):
    """mylsd::createMapCache (LSD/myLSD.h:131, LSD/myLSD.cpp:11): CV_64FC1-like float64 array, metres, capped at
    z_occ_max_dis.  Call it before myLineSegmentDetector, which rewrites MapGray."""
    return (ctx or default_context()).map_cache(MapGray, res, z_occ_max_dis)


# FeatureAssociation constants, LSD/baseFunc.h:80-86
ignoreScanLength, scanToMapDiff, maxEstiDist = 40, 0.35, 60


def match_pairs(map_lines, scan_lines):
    """The (cntMapLine, cntScanLine) pairs FeatureAssociation hands to its thread pool (LSD/myFA.cpp:28-58), in its order."""
    pairs = []
    for cs in range(len(scan_lines)):
        ls = float(scan_lines["len"][cs])
        if ls < ignoreScanLength:
            continue
        ld = ls * scanToMapDiff
        for cm in range(len(map_lines)):
            lm = float(map_lines["len"][cm])
            if lm < ls - ld or lm > ls + ld:
                continue
            pairs.append((cm, cs))
    return np.array(pairs, np.int32).reshape(-1, 2)


def FeatureScan(mapParam, lidarPointPolar, RegionPointLimitNumber=rdp_leastPoint, threLine=rdp_threLine, lineDistThreM=rdp_leastDist, ctx=None):
    """myrdp::FeatureScan (LSD/myRDP.cpp:9) for one scan: mapParam = (oriMapCol, oriMapRow, mapResol, mapOriX, mapOriY), lidarPointPolar float64
    [len_lp, 2] = (range, angle) of the finite readings (the caller's read loop drops the infinite ones, LSD/main_on_windows.cpp:115-121).
    Returns dict(linesInfo, len_linesInfo, scanImPoint [m, 3], lidarPos (x, y), lineIm) -- structFeatureScan (LSD/myRDP.h:55-61)."""
    own = ctx is None
    ctx = ctx or Context(0)
    try:
        sc = np.ascontiguousarray(lidarPointPolar, np.float64).reshape(1, -1, 2)
        return ctx.feature_scan_batch(sc, [sc.shape[1]], mapParam, RegionPointLimitNumber, threLine, lineDistThreM)[0]
    finally:
        if own:
            ctx.close()


def ScanToMapMatch(mapCache, mapLinesInfo, scanLinesInfo, scanImPoint, lidarPose, lastPose, ctx=None):
    """The matching stage of myfa::FeatureAssociation (LSD/myFA.cpp:28-100): every admissible (scan line, map line) pair x 4
    matchings scored on the device, candidates with score < 3 kept (:262) and sorted by score (:98, CompScore :398-402).
    Returns SCORE_DTYPE records (the reference's structScore without the debug pointer)."""
    pairs = match_pairs(mapLinesInfo, scanLinesInfo)
    if len(pairs) == 0:
        return np.zeros(0, SCORE_DTYPE)
    sc = (ctx or default_context()).scan_to_map_match(mapCache, mapLinesInfo, scanLinesInfo, scanImPoint, lidarPose, lastPose, pairs,
                                                      z_occ_max_dis, maxEstiDist).ravel()
    keep = sc[sc["score"] < 3]
    return keep[np.argsort(keep["score"], kind="stable")]


def _pos(p):
    return lsd_position(float(p[0]), float(p[1]), float(p[2]) if len(p) > 2 else 0.0)


def _map_param(mp):
    return lsd_map_param(int(mp[0]), int(mp[1]), float(mp[2]), float(mp[3]), float(mp[4]))


def _host_scans(scans, lens, poses):
    """The host arrays every grid method takes, contiguous: scans float64 [n, stride, 2], lens int32 [n], poses float64 [n, 3]; and whether
    they have those shapes."""
    sc = np.ascontiguousarray(scans, np.float64)
    ln = np.ascontiguousarray(lens, np.int32).reshape(-1)
    po = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
    return sc, ln, po, sc.ndim == 3 and sc.shape[2] == 2 and sc.shape[0] == len(ln) and len(po) == len(ln)


def _u32s(*values, limit):
    """Counts as the C ABI's unsigned arguments take them: integers in 0 .. limit - 1 (ctypes would wrap anything else silently)."""
    out = tuple(int(v) for v in values)
    if any(not 0 <= v < m for v, m in zip(out, limit)):
        raise LsdError(LSD_ERR_INVALID, "a count outside its unsigned range: %r" % (out,))
    return out


def grid_smear_default(sigma_cells=1.0, radius=3):
    """lsd_grid_smear_default: the table w[|v|][|u|] = floor(255 * exp(-(u^2 + v^2) / (2 sigma_cells^2)) + 0.5) within `radius`, 0 elsewhere."""
    out = lsd_grid_smear()
    st = load_library().lsd_grid_smear_default(float(sigma_cells), int(radius), C.byref(out))
    if st != LSD_OK:
        raise LsdError(st, "grid_smear_default: sigma_cells > 0 and finite, radius 0..7")
    return out


def grid_smear(smear=None):
    """An lsd_grid_smear: `smear` itself, (radius, w) with w an 8 x 8 table of 0..255 indexed [|dv|][|du|], or None: the default table."""
    if isinstance(smear, lsd_grid_smear):
        return smear
    if smear is None:
        return grid_smear_default(1.0, 3)
    radius, w = smear
    w = np.asarray(w)
    if w.shape != (8, 8) or (w < 0).any() or (w > 255).any():
        raise LsdError(LSD_ERR_INVALID, "a smear table is 8 x 8 values of 0..255")
    out = lsd_grid_smear()
    out.radius = int(radius)
    C.memmove(out.w, np.ascontiguousarray(w, np.uint8).ctypes.data, 64)
    return out


def grid_smear_table(smear):
    """(radius, the 8 x 8 uint8 table) of an lsd_grid_smear."""
    return int(smear.radius), np.frombuffer(bytes(smear.w), np.uint8).reshape(8, 8).copy()


def grid_search(search=None, **kw):
    """An lsd_grid_search: `search` itself, a dict or a tuple (wx, wy, na, ang_step, min_beams, min_num, min_den), or keywords.  The window
    is +-wx, +-wy cells and +-na steps of ang_step degrees; a match is accepted with at least min_beams scored beams and a mean response
    of at least 255 * min_num / min_den."""
    if isinstance(search, lsd_grid_search):
        return search
    if isinstance(search, dict):
        kw = dict(search, **kw)
        search = None
    if search is None:
        a = dict(wx=3, wy=3, na=2, ang_step=0.5, min_beams=30, min_num=1, min_den=4)
        a.update(kw)
        search = tuple(a[k] for k in ("wx", "wy", "na", "ang_step", "min_beams", "min_num", "min_den"))
    wx, wy, na, step, mb, mn, md = search
    mb, mn, md = _u32s(mb, mn, md, limit=(1 << 32,) * 3)
    return lsd_grid_search(int(wx), int(wy), int(na), float(step), mb, mn, md)


GRID_LOCATE_KEYS = ("x0", "y0", "nx", "ny", "ang0", "ang_step", "n_ang", "levels", "max_nodes", "score_floor", "min_beams", "min_num", "min_den")


def grid_locate_tight(tight):
    """The flag word of a `tight=` argument: None, 0 or False the existing search (0); True both flags; "probe" or "retry" one of them; or
    a word of GRID_LOCATE_TIGHT_PROBE | GRID_LOCATE_TIGHT_RETRY."""
    if tight is None or tight is False:
        return 0
    if tight is True:
        return GRID_LOCATE_TIGHT_PROBE | GRID_LOCATE_TIGHT_RETRY
    if isinstance(tight, str):
        if tight not in ("probe", "retry"):
            raise LsdError(LSD_ERR_INVALID, 'tight: "probe" or "retry"')
        return GRID_LOCATE_TIGHT_PROBE if tight == "probe" else GRID_LOCATE_TIGHT_RETRY
    if not isinstance(tight, (int, np.integer)) or not 0 <= int(tight) <= 3:
        raise LsdError(LSD_ERR_INVALID, "tight: None, a bool, \"probe\", \"retry\" or a word of GRID_LOCATE_TIGHT_PROBE | GRID_LOCATE_TIGHT_RETRY")
    return int(tight)


def grid_locate(locate=None, cols=None, rows=None, **kw):
    """An lsd_grid_locate_par: `locate` itself, a dict or a tuple of GRID_LOCATE_KEYS, or keywords.  The box is nx x ny lidar cells from
    (x0, y0) -- by default the whole grid, which takes cols and rows (the methods of a GridMapper and of a Context pass their own) --, the
    headings ang0 + a * ang_step degrees for a < n_ang; the search runs over `levels` pyramid levels with at most max_nodes nodes alive
    per level; a location is accepted with at least min_beams scored beams and a mean response of at least 255 * min_num / min_den.
    The defaults of levels (4), max_nodes (2^20), n_ang and ang_step (360 headings of 1 degree) are PLACEHOLDERS: nobody has measured
    which suit real maps (DESIGN.md 8.1.12 has what the probe found on generated rooms)."""
    if isinstance(locate, lsd_grid_locate_par):
        return locate
    if isinstance(locate, dict):
        kw = dict(locate, **kw)
        locate = None
    if locate is None or locate is True:
        a = dict(x0=0, y0=0, nx=cols, ny=rows, ang0=0.0, ang_step=1.0, n_ang=360, levels=4, max_nodes=1 << 20, score_floor=0, min_beams=30,
                 min_num=1, min_den=4)
        unknown = set(kw) - set(a)
        if unknown:
            raise LsdError(LSD_ERR_INVALID, "grid_locate: unknown keys %s" % sorted(unknown))
        a.update(kw)
        if a["nx"] is None or a["ny"] is None:
            raise LsdError(LSD_ERR_INVALID, "grid_locate: the default box is the whole grid; give nx and ny where no grid is known")
        locate = tuple(a[k] for k in GRID_LOCATE_KEYS)
    x0, y0, nx, ny, ang0, step, n_ang, levels, mx, fl, mb, mn, md = locate
    mx, fl, mb, mn, md = _u32s(mx, fl, mb, mn, md, limit=(1 << 32,) * 5)
    return lsd_grid_locate_par(int(x0), int(y0), int(nx), int(ny), float(ang0), float(step), int(n_ang), int(levels), mx, fl, mb, mn, md)


def grid_pyramid_bytes(cols, rows, levels):
    """lsd_grid_pyramid_bytes: the size of the pyramid buffer of a cols x rows lookup plane with the levels 0..levels (0: refused)."""
    return int(load_library().lsd_grid_pyramid_bytes(int(cols), int(rows), int(levels)))


def grid_pyramid_offset(cols, rows, h):
    """lsd_grid_pyramid_offset: where level h starts in the pyramid buffer."""
    return int(load_library().lsd_grid_pyramid_offset(int(cols), int(rows), int(h)))


def grid_response(response=None, rx=3, ry=3, ra=1, keep=(1, 2)):
    """An lsd_grid_response: `response` itself, a dict of rx / ry / ra / keep (or keep_num, keep_den), a tuple (rx, ry, ra, keep_num,
    keep_den), or keywords.  The neighbourhood is +-rx, +-ry cells and +-ra angle steps around the winner; a candidate enters the
    covariance iff its score is at least keep[0] / keep[1] of the winner's."""
    if isinstance(response, lsd_grid_response):
        return response
    if isinstance(response, dict):
        a = dict(response)
        if "keep" in a:
            a["keep_num"], a["keep_den"] = a.pop("keep")
        response = (a.get("rx", rx), a.get("ry", ry), a.get("ra", ra), a.get("keep_num", keep[0]), a.get("keep_den", keep[1]))
    if response is None or response is True:
        response = (rx, ry, ra, keep[0], keep[1])
    rx, ry, ra, kn, kd = response
    kn, kd = _u32s(kn, kd, limit=(1 << 32,) * 2)
    return lsd_grid_response(int(rx), int(ry), int(ra), kn, kd)


def grid_ray(ray=None, tol=None, drop=("short",), min_beams=1, ok=(1, 2), gate=False, mapResol=None):
    """An lsd_grid_ray_par: `ray` itself, a dict of tol / drop (or drop_mask) / min_beams / ok (or ok_num, ok_den) / gate, a tuple (tol,
    drop_mask, min_beams, ok_num, ok_den, gate), or keywords.  A beam agrees with the map iff its range is within tol metres of the
    expected one; drop: the classes (names of GRID_RAY_CLASSES or their numbers) whose readings a screened scan loses; a scan is
    consistent with at least min_beams judged beams of which ok[0] / ok[1] agree; gate: a cast scan that is not consistent loses its
    pose.  tol=None means two cells of the mapper's mapResol and is resolved where the mapper is known (mapResol given); elsewhere it is
    refused."""
    if isinstance(ray, lsd_grid_ray_par):
        return ray
    if isinstance(ray, dict):
        a = dict(ray)
        if "ok" in a:
            a["ok_num"], a["ok_den"] = a.pop("ok")
        ray = (a.get("tol", tol), a.get("drop_mask", a.get("drop", drop)), a.get("min_beams", min_beams), a.get("ok_num", ok[0]),
               a.get("ok_den", ok[1]), a.get("gate", gate))
    if ray is None or ray is True:
        ray = (tol, drop, min_beams, ok[0], ok[1], gate)
    tol, mask, mb, on, od, gate = ray
    if tol is None:
        if mapResol is None:
            raise LsdError(LSD_ERR_INVALID, "grid_ray: tol=None is two cells of a mapper's mapResol; give tol where no mapper is known")
        tol = 2 * float(mapResol)
    if not isinstance(mask, (int, np.integer)):
        names = [GRID_RAY_CLASSES.index(c) if isinstance(c, str) and c in GRID_RAY_CLASSES else c for c in mask]
        if any(not isinstance(c, (int, np.integer)) or not 0 <= c < 7 for c in names):
            raise LsdError(LSD_ERR_INVALID, "grid_ray: drop names classes of GRID_RAY_CLASSES or their numbers 0..6")
        mask = sum({1 << int(c) for c in names})
    mask, mb, on, od = _u32s(mask, mb, on, od, limit=(1 << 32,) * 4)
    return lsd_grid_ray_par(float(tol), mask, mb, on, od, 1 if gate else 0)


def fa_correct(correct=None, cov_scale=1.0, floor_xy=1.0, floor_ang=1.0, gate=0.0):
    """An lsd_fa_correct: `correct` itself, a dict of cov_scale / floor_xy / floor_ang / gate, a tuple of the four in that order, or
    keywords (None / True: the defaults).  R = the response's covariance x cov_scale + the floors on its diagonal (pixels^2, pixels^2,
    degrees^2; the defaults are the reference filter's own R = I); gate > 0 refuses a correction whose squared Mahalanobis distance
    exceeds it (0: no gate, as the reference has none).  LsdError(LSD_ERR_INVALID) for a value that is not finite or negative."""
    if isinstance(correct, lsd_fa_correct):
        return correct
    if isinstance(correct, dict):
        a = dict(correct)
        correct = (a.get("cov_scale", cov_scale), a.get("floor_xy", floor_xy), a.get("floor_ang", floor_ang), a.get("gate", gate))
    if correct is None or correct is True:
        correct = (cov_scale, floor_xy, floor_ang, gate)
    vals = tuple(float(v) for v in correct)
    if len(vals) != 4 or not all(np.isfinite(v) and v >= 0 for v in vals):
        raise LsdError(LSD_ERR_INVALID, "cov_scale, floor_xy, floor_ang and gate must be finite and >= 0")
    return lsd_fa_correct(*vals)


def _pg_par(cls, given, defaults, kw):
    """A parameter struct of the pose graph: `given` itself, or a dict over the defaults, or keywords; the C entries do the refusing."""
    if isinstance(given, cls):
        return given
    a = dict(defaults)
    a.update({k: v for k, v in kw.items() if v is not None})
    if isinstance(given, dict):
        unknown = set(given) - set(a)
        if unknown:
            raise LsdError(LSD_ERR_INVALID, "%s: unknown keys %s" % (cls.__name__, sorted(unknown)))
        a.update(given)
    elif given is not None and given is not True:
        raise LsdError(LSD_ERR_INVALID, "%s takes a dict, keywords or the struct itself" % cls.__name__)
    return a


PG_APPEND_DEFAULTS = dict(min_dist=4.0, min_ang=10.0, info=(1.0, 0.0, 1.0, 0.0, 0.0, 1.0))
PG_CLOSURE_DEFAULTS = dict(cov_scale=1.0, floor_xy=1.0, floor_ang=1.0)
PG_RELAX_DEFAULTS = dict(lambda0=1e-3, lambda_min=1e-9, up=10.0, down=10.0, cg_tol=1e-8, eps=1e-9, iters=20, cg_iters=200)


def pg_append(append=None, min_dist=None, min_ang=None, info=None):
    """An lsd_pg_append: a frame becomes a keyframe once it is min_dist pixels or min_ang degrees from the last one; info is the
    information of an odometry edge (xx, xy, yy, xa, ya, aa; 1 / pixels^2 and 1 / degrees^2)."""
    a = _pg_par(lsd_pg_append, append, PG_APPEND_DEFAULTS, dict(min_dist=min_dist, min_ang=min_ang, info=info))
    if isinstance(a, lsd_pg_append):
        return a
    inf = tuple(float(v) for v in a["info"])
    if len(inf) != 6:
        raise LsdError(LSD_ERR_INVALID, "info is xx, xy, yy, xa, ya, aa")
    return lsd_pg_append(float(a["min_dist"]), float(a["min_ang"]), (C.c_double * 6)(*inf))


def pg_closure(closure=None, cov_scale=None, floor_xy=None, floor_ang=None):
    """An lsd_pg_closure: R = the response's covariance x cov_scale + the floors on its diagonal, as fa_correct()'s; the closure edge's
    information is its inverse in the anchor's frame."""
    a = _pg_par(lsd_pg_closure, closure, PG_CLOSURE_DEFAULTS, dict(cov_scale=cov_scale, floor_xy=floor_xy, floor_ang=floor_ang))
    return a if isinstance(a, lsd_pg_closure) else lsd_pg_closure(float(a["cov_scale"]), float(a["floor_xy"]), float(a["floor_ang"]))


def pg_relax(relax=None, lambda0=None, lambda_min=None, up=None, down=None, cg_tol=None, eps=None, iters=None, cg_iters=None):
    """An lsd_pg_relax: Levenberg-Marquardt's damping (lambda0, divided by `down` after an accepted step but never below lambda_min,
    multiplied by `up` after a rejected one), at most `iters` outer iterations of at most cg_iters conjugate-gradient steps each, which
    end once r.z <= cg_tol^2 of its start; an accepted step whose largest component is below eps ends the call."""
    a = _pg_par(lsd_pg_relax, relax, PG_RELAX_DEFAULTS, dict(lambda0=lambda0, lambda_min=lambda_min, up=up, down=down, cg_tol=cg_tol, eps=eps,
                                                              iters=iters, cg_iters=cg_iters))
    if isinstance(a, lsd_pg_relax):
        return a
    it, cg = int(a["iters"]), int(a["cg_iters"])
    if not (-2 ** 31 <= it < 2 ** 31 and -2 ** 31 <= cg < 2 ** 31):
        raise LsdError(LSD_ERR_INVALID, "iters and cg_iters are int32")
    return lsd_pg_relax(*(float(a[k]) for k in ("lambda0", "lambda_min", "up", "down", "cg_tol", "eps")), it, cg)


PG_ROBUST_DEFAULTS = dict(kernel="huber", delta=1.0, scope="closures")
_PG_KERNELS = {"none": PG_KERNEL_NONE, "huber": PG_KERNEL_HUBER, "gm": PG_KERNEL_GM}
_PG_SCOPES = {"closures": PG_ROBUST_CLOSURES, "all": PG_ROBUST_ALL}


def pg_robust(robust=None, kernel=None, delta=None, scope=None):
    """An lsd_pg_robust: the kernel on the edges of a robust relaxation -- "huber" (for a first relaxation from drifted poses), "gm"
    (Geman-McClure: for a closure that arrives on a graph that is already relaxed), "none" or the C side's number --, its width delta
    in units of sqrt(chi2), and the scope: "closures" (edges with PG_EDGE_CLOSURE) or "all".  DESIGN.md 8.1.16 has the cases."""
    a = _pg_par(lsd_pg_robust, robust, PG_ROBUST_DEFAULTS, dict(kernel=kernel, delta=delta, scope=scope))
    if isinstance(a, lsd_pg_robust):
        return a
    k, s = a["kernel"], a["scope"]
    if isinstance(k, str) and k not in _PG_KERNELS or isinstance(s, str) and s not in _PG_SCOPES:
        raise LsdError(LSD_ERR_INVALID, "kernel is one of %s or an int, scope one of %s or an int" % (sorted(_PG_KERNELS), sorted(_PG_SCOPES)))
    k, s = int(_PG_KERNELS.get(k, k)), int(_PG_SCOPES.get(s, s))
    if not (-2 ** 31 <= k < 2 ** 31 and 0 <= s < 2 ** 32):
        raise LsdError(LSD_ERR_INVALID, "kernel is int32, scope uint32")
    return lsd_pg_robust(k, s, float(a["delta"]))


_PG_PRECONDS = {"block": PG_PRECOND_BLOCK, "chain": PG_PRECOND_CHAIN}


def pg_precond(precond=None, kind=None):
    """An lsd_pg_precond: the preconditioner of the relaxation's conjugate gradients -- "block" (the inverse 3 x 3 diagonal blocks: the
    default of every entry), "chain" (the block-tridiagonal part of the normal matrix along the odometry chains) or
    the C side's number."""
    if isinstance(precond, lsd_pg_precond):
        return precond
    k = kind if kind is not None else ("block" if precond is None else precond)
    if isinstance(k, dict):
        if set(k) - {"kind"}:
            raise LsdError(LSD_ERR_INVALID, "lsd_pg_precond: unknown keys %s" % sorted(set(k) - {"kind"}))
        k = k.get("kind", "block")
    if isinstance(k, str) and k not in _PG_PRECONDS:
        raise LsdError(LSD_ERR_INVALID, "precond is one of %s or an int" % sorted(_PG_PRECONDS))
    k = int(_PG_PRECONDS.get(k, k))
    if not -2 ** 31 <= k < 2 ** 31:
        raise LsdError(LSD_ERR_INVALID, "precond is int32")
    return lsd_pg_precond(k, 0)


PG_PLACE_DEFAULTS = dict(gap=10, window=2, spread=2, k=4, pick=0, max_dist=1024, min_sectors=16)


def pg_place(place=None, gap=None, window=None, spread=None, k=None, pick=None, max_dist=None, min_sectors=None):
    """An lsd_pg_place: place recognition's parameters -- a candidate is at least `gap` nodes older than the query, has at least
    min_sectors sectors with a return and a descriptor distance of at most max_dist (0..16320: 64 sectors of 0..255); the k (1..8) best
    are reported, each suppressing the nodes within `spread` of it; round `pick` is the place that is matched, with the nodes within
    `window` of it drawn as its neighbourhood.  DESIGN.md 8.1.17."""
    a = _pg_par(lsd_pg_place, place, PG_PLACE_DEFAULTS, dict(gap=gap, window=window, spread=spread, k=k, pick=pick, max_dist=max_dist,
                                                             min_sectors=min_sectors))
    if isinstance(a, lsd_pg_place):
        return a
    ints = [int(a[n]) for n in ("gap", "window", "spread", "k", "pick")]
    us = [int(a[n]) for n in ("max_dist", "min_sectors")]
    if not all(-2 ** 31 <= v < 2 ** 31 for v in ints) or not all(0 <= v < 2 ** 32 for v in us):
        raise LsdError(LSD_ERR_INVALID, "gap, window, spread, k and pick are int32, max_dist and min_sectors uint32")
    return lsd_pg_place(*ints, *us, 0)


PG_LOOPS_DEFAULTS = dict(max_loops=8, spread=2)


def pg_loops(loops=None, max_loops=None, spread=None):
    """An lsd_pg_loops: at most max_loops (1..64) distinct loops are chosen among the records of a batch of queries; a chosen loop
    (query, anchor) suppresses every pair within `spread` of it on both axes, and a pair that near to a closure edge the graph already
    has is left out.  DESIGN.md 8.1.18."""
    a = _pg_par(lsd_pg_loops, loops, PG_LOOPS_DEFAULTS, dict(max_loops=max_loops, spread=spread))
    if isinstance(a, lsd_pg_loops):
        return a
    ints = [int(a[n]) for n in ("max_loops", "spread")]
    if not all(-2 ** 31 <= v < 2 ** 31 for v in ints):
        raise LsdError(LSD_ERR_INVALID, "max_loops and spread are int32")
    return lsd_pg_loops(*ints)


PG_REDUCE_DEFAULTS = dict(cell=4.0, ang_bin=10.0, keep=1, max_run=64)


def pg_reduce(reduce=None, cell=None, ang_bin=None, keep=None, max_run=None):
    """An lsd_pg_reduce: a keyframe is redundant where `keep` older ones lie in its cell of `cell` pixels by `ang_bin` degrees (about the
    append's min_dist and min_ang: the keyframe spacing); at most max_run nodes in a row are contracted into one edge.  DESIGN.md
    8.1.21."""
    a = _pg_par(lsd_pg_reduce, reduce, PG_REDUCE_DEFAULTS, dict(cell=cell, ang_bin=ang_bin, keep=keep, max_run=max_run))
    if isinstance(a, lsd_pg_reduce):
        return a
    ints = [int(a[n]) for n in ("keep", "max_run")]
    if not all(-2 ** 31 <= v < 2 ** 31 for v in ints):
        raise LsdError(LSD_ERR_INVALID, "keep and max_run are int32")
    return lsd_pg_reduce(float(a["cell"]), float(a["ang_bin"]), *ints)


def pg_reduce_workspace_bytes(nodes_cap, edges_cap, store_stride):
    """lsd_pg_reduce_workspace_bytes: the workspace of enqueue_pg_reduce_device; 0 for arguments outside the limits."""
    return int(load_library().lsd_pg_reduce_workspace_bytes(int(nodes_cap), int(edges_cap), int(store_stride)))


def pg_loops_workspace_bytes(n_q, k, edges_cap):
    """lsd_pg_loops_workspace_bytes: the workspace of enqueue_pg_loops_device; 0 for arguments it refuses."""
    return int(load_library().lsd_pg_loops_workspace_bytes(int(n_q), int(k), int(edges_cap)))


def pg_workspace_pc_bytes(nodes_cap, edges_cap, precond):
    """lsd_pg_workspace_pc_bytes: the workspace of ONE graph of enqueue_pg_relax_pc_device for a preconditioner (pg_precond()); 0 for
    caps or a kind outside the limits."""
    return int(load_library().lsd_pg_workspace_pc_bytes(int(nodes_cap), int(edges_cap), int(pg_precond(precond).kind)))


PG_MARG_DEFAULTS = dict(cg_tol=1e-8, cg_iters=200, precond="chain", slots=256)


def pg_marg(marg=None, cg_tol=None, cg_iters=None, precond=None, slots=None):
    """An lsd_pg_marg: the solves behind marginal covariances -- at most cg_iters conjugate-gradient steps per column, ended once r.z <=
    cg_tol^2 of its start; precond as pg_precond() ("chain" by default: a track's matrix is a chain plus a few closures); slots (1..1024):
    how many workgroups share the queries, each with vectors of its own in the workspace.  A record does not depend on slots."""
    a = _pg_par(lsd_pg_marg, marg, PG_MARG_DEFAULTS, dict(cg_tol=cg_tol, cg_iters=cg_iters, precond=precond, slots=slots))
    if isinstance(a, lsd_pg_marg):
        return a
    cg, sl = int(a["cg_iters"]), int(a["slots"])
    if not (-2 ** 31 <= cg < 2 ** 31 and -2 ** 31 <= sl < 2 ** 31):
        raise LsdError(LSD_ERR_INVALID, "cg_iters and slots are int32")
    return lsd_pg_marg(float(a["cg_tol"]), cg, int(pg_precond(a["precond"]).kind), sl, 0)


def pg_queries(queries):
    """Queries of the marginals as PG_MARG_QUERY_DTYPE [n]: such an array itself, or rows (kind, a, b) of integers."""
    if isinstance(queries, np.ndarray) and queries.dtype == PG_MARG_QUERY_DTYPE:
        return np.ascontiguousarray(queries).reshape(-1)
    q = np.asarray(queries, dtype=np.int64).reshape(-1, 3)
    if len(q) and (q.min() < -2 ** 31 or q.max() >= 2 ** 31):
        raise LsdError(LSD_ERR_INVALID, "kind, a and b are int32")
    out = np.zeros(len(q), PG_MARG_QUERY_DTYPE)
    out["kind"], out["a"], out["b"] = q[:, 0], q[:, 1], q[:, 2]
    return out


def pg_vet(vet=None, gate=None, marg=None):
    """The setting of a vetted closure chain (PoseGraph.close_device(.., vet=) and its kin): {"gate": the bound on the closure's squared
    Mahalanobis distance under the pair's covariance plus its own -- 16.27 is the 0.999 quantile of chi-square with 3 degrees of freedom
    --, "marg": pg_marg()}."""
    a = dict(gate=16.27, marg=None)
    if isinstance(vet, dict):
        if set(vet) - set(a):
            raise LsdError(LSD_ERR_INVALID, "vet: unknown keys %s" % sorted(set(vet) - set(a)))
        a.update(vet)
    elif vet is not None and vet is not True:
        raise LsdError(LSD_ERR_INVALID, "vet takes a dict or keywords")
    a.update({k: v for k, v in dict(gate=gate, marg=marg).items() if v is not None})
    return dict(gate=float(a["gate"]), marg=pg_marg(a["marg"]))


def pg_marginals_workspace_bytes(nodes_cap, edges_cap, precond, slots):
    """lsd_pg_marginals_workspace_bytes: pg_workspace_pc_bytes plus one slice of vectors per slot; 0 for arguments outside the limits."""
    return int(load_library().lsd_pg_marginals_workspace_bytes(int(nodes_cap), int(edges_cap), int(pg_precond(precond).kind), int(slots)))


def pg_workspace_bytes(nodes_cap, edges_cap):
    """lsd_pg_workspace_bytes: the workspace of ONE graph of the relaxation; 0 for caps outside 1..16384 / 1..65536."""
    return int(load_library().lsd_pg_workspace_bytes(int(nodes_cap), int(edges_cap)))


FA_SEED_KEYS = ("var_xy", "var_ang", "cov_scale", "floor_xy", "floor_ang", "max_best")


def fa_seed(seed=None, var_xy=1.0, var_ang=1.0, cov_scale=1.0, floor_xy=1.0, floor_ang=1.0, max_best=1):
    """An lsd_fa_seed: `seed` itself, a dict of FA_SEED_KEYS, a tuple of the six in that order, or keywords (None / True: the defaults).
    Without response records the seeded covariance of (x, y, ang) is diag(var_xy, var_xy, var_ang) (pixels^2, pixels^2, degrees^2; the
    search's own resolution, one cell and one degree, by default); with them it is the response's covariance x cov_scale + the floors, as
    fa_correct()'s R.  max_best: the most equal winners (the locate record's n_best) a seed accepts; 1 refuses every tie.
    LsdError(LSD_ERR_INVALID) for a real value that is not finite or negative, or max_best outside 1..2^32-1."""
    if isinstance(seed, lsd_fa_seed):
        return seed
    if isinstance(seed, dict):
        a = dict(var_xy=var_xy, var_ang=var_ang, cov_scale=cov_scale, floor_xy=floor_xy, floor_ang=floor_ang, max_best=max_best)
        unknown = set(seed) - set(a)
        if unknown:
            raise LsdError(LSD_ERR_INVALID, "fa_seed: unknown keys %s" % sorted(unknown))
        a.update(seed)
        seed = tuple(a[k] for k in FA_SEED_KEYS)
    if seed is None or seed is True:
        seed = (var_xy, var_ang, cov_scale, floor_xy, floor_ang, max_best)
    if len(seed) != 6:
        raise LsdError(LSD_ERR_INVALID, "fa_seed takes var_xy, var_ang, cov_scale, floor_xy, floor_ang, max_best")
    vals = tuple(float(v) for v in seed[:5])
    if not all(np.isfinite(v) and v >= 0 for v in vals):
        raise LsdError(LSD_ERR_INVALID, "var_xy, var_ang, cov_scale, floor_xy and floor_ang must be finite and >= 0")
    mb, = _u32s(seed[5], limit=(1 << 32,))
    if mb == 0:
        raise LsdError(LSD_ERR_INVALID, "max_best must be at least 1")
    return lsd_fa_seed(*vals, mb, 0)


def map_frame(frame):
    """An lsd_map_frame from (mapResol, mapOriX, mapOriY), from a map_param (oriMapCol, oriMapRow, mapResol, mapOriX, mapOriY) or from an
    lsd_map_frame; LsdError(LSD_ERR_INVALID) for a resolution that is not finite and > 0 or an origin that is not finite."""
    if isinstance(frame, lsd_map_frame):
        v = (frame.mapResol, frame.mapOriX, frame.mapOriY)
    else:
        v = tuple(float(x) for x in frame)
        if len(v) == 5:
            v = v[2:]
    if len(v) != 3:
        raise LsdError(LSD_ERR_INVALID, "a map frame is (mapResol, mapOriX, mapOriY)")
    if not (np.isfinite(v[0]) and v[0] > 0 and np.isfinite(v[1]) and np.isfinite(v[2])):
        raise LsdError(LSD_ERR_INVALID, "a map frame needs a finite mapResol > 0 and a finite origin, not %r" % (v,))
    return lsd_map_frame(*v)


def map_ref(d_map_cache, cols, rows, d_map_lines, n_map, map_param, d_n_map=0):
    """One MAP_REF_DTYPE record: device addresses (integers) of the cache, the line records and -- or 0 -- the device-side line count,
    the geometry, and mapResol / mapOriX / mapOriY from map_param = (oriMapCol, oriMapRow, mapResol, mapOriX, mapOriY)."""
    r = np.zeros(1, MAP_REF_DTYPE)[0]
    r["d_map_cache"], r["d_map_lines"], r["d_n_map"] = int(d_map_cache or 0), int(d_map_lines or 0), int(d_n_map or 0)
    r["cols"], r["rows"], r["n_map"] = int(cols), int(rows), int(n_map)
    r["mapResol"], r["mapOriX"], r["mapOriY"] = float(map_param[2]), float(map_param[3]), float(map_param[4])
    return r


def map_table(maps):
    """The host table the fleet entries take: a contiguous MAP_REF_DTYPE array from an array or a sequence of map_ref records."""
    if isinstance(maps, np.ndarray) and maps.dtype == MAP_REF_DTYPE:
        return np.ascontiguousarray(maps).reshape(-1)
    return np.array(list(maps), MAP_REF_DTYPE).reshape(-1)


def fa_state(state):
    """An FA_STATE_DTYPE array of one record from a record, or from (kalman_x [9], kalman_P [9, 9] indexed P[i, j])."""
    if isinstance(state, np.void) or (isinstance(state, np.ndarray) and state.dtype == FA_STATE_DTYPE):
        return np.ascontiguousarray(np.asarray(state, FA_STATE_DTYPE).reshape(1))
    x, P = state
    st = np.zeros(1, FA_STATE_DTYPE)
    st["x"][0] = np.asarray(x, np.float64).reshape(9)
    st["P"][0] = np.asarray(P, np.float64).reshape(9, 9).ravel(order="F")      # column-major, as Eigen stores it
    return st


def load_odom(path_or_rows):
    """The replay driver's Odom vector (LSD/main_on_windows.cpp:51-61) from Odom.txt (or its rows float64 [n, 3]): the feof loop
    appends one more row after the last line (the file ends in a newline; fscanf then leaves the row as it was -- taken here to
    repeat the last row, an assumption: the reference leaves it uninitialised), and Odom[0].x = 0.  A log of n lidar frames
    has n rows, so the vector has n + 1 and the last frame sees a zero odometry step."""
    rows = np.loadtxt(path_or_rows).reshape(-1, 3) if isinstance(path_or_rows, str) else np.asarray(path_or_rows, np.float64).reshape(-1, 3)
    od = np.concatenate([rows, rows[-1:]], 0)
    od[0, 0] = 0.0
    return od


def lidar_frames(lidar):
    """The driver's read loop (LSD/main_on_windows.cpp:104-123) on float64 [n, B, 2] (range, angle) frames (the reference's B: 360):
    readings with an infinite range dropped.  Returns (scans [n, B, 2] with the finite readings first, lens int32 [n])."""
    lid = np.asarray(lidar, np.float64)
    scans = np.zeros_like(lid)
    lens = np.zeros(len(lid), np.int32)
    for f in range(len(lid)):
        keep = lid[f][lid[f, :, 0] != np.inf]
        scans[f, :len(keep)] = keep
        lens[f] = len(keep)
    return scans, lens


def FeatureAssociation(mapCache, mapLinesInfo, scanLinesInfo, scanImPoint, lidarPose, lastPose, kalman_x, kalman_P, ScanPose, ctx=None):
    """myfa::FeatureAssociation (LSD/myFA.cpp:13) on the FAInput fields: returns (kalman_x [9], kalman_P [9, 9], report)."""
    st, rep = (ctx or default_context()).feature_association(mapCache, mapLinesInfo, scanLinesInfo, scanImPoint, lidarPose, lastPose, ScanPose,
                                                             (kalman_x, kalman_P))
    return st["x"].copy(), st["P"].reshape(9, 9, order="F").copy(), rep


def replay_log(map_u8, map_param, lidar, odom, ctx=None):
    """The replay driver (LSD/main_on_windows.cpp:24-186) on the device: mapCache and the map lines of map_u8 (a copy: the LSD call
    rewrites it), then FeatureScan and FeatureAssociation for every lidar frame.  lidar float64 [n, 360, 2] as in Lidar.txt, odom the
    Odom vector (load_odom, n + 1 rows).  Returns (states FA_STATE_DTYPE [n], reports FA_REPORT_DTYPE [n]); the trajectory is
    states["x"][:, :3]."""
    cx = ctx or default_context()
    m = np.ascontiguousarray(map_u8, np.uint8).copy()
    mapCache = cx.map_cache(m, float(map_param[2]), z_occ_max_dis)
    LSD = myLineSegmentDetector(m, m.shape[1], m.shape[0], lsd_sca, lsd_sig, lsd_angThre, lsd_denThre, pseBin, ctx=cx)
    scans, lens = lidar_frames(lidar)
    return cx.localize(mapCache, LSD.linesInfo, scans, lens, odom, map_param)


def lidar_frames_batch(lidar):
    """lidar_frames on float64 [..., B, 2] frames at once (the same rule and the same output, vectorised)."""
    lid = np.asarray(lidar, np.float64)
    keep = lid[..., 0] != np.inf
    order = np.argsort(~keep, axis=-1, kind="stable")                        # the finite readings first, in their order
    scans = np.take_along_axis(lid, order[..., None], axis=-2)
    lens = keep.sum(-1).astype(np.int32)
    scans[np.arange(lid.shape[-2]) >= lens[..., None]] = 0.0
    return scans, lens


def _cuda_stream(stream):
    """The torch stream an enqueue goes on: `stream`, or the current one."""
    import torch
    if stream is None:
        return torch.cuda.current_stream()
    if not isinstance(stream, torch.cuda.Stream):
        raise LsdError(LSD_ERR_INVALID, "stream must be a torch.cuda.Stream (or None: the current stream)")
    return stream


def _occupancy_grid(d_grid, cols, rows, device):
    """d_grid as the map update reads it: a contiguous CUDA int8 tensor of rows * cols cells (flat, or [rows, cols]) on `device`."""
    import torch
    if not isinstance(d_grid, torch.Tensor) or not d_grid.is_cuda or d_grid.dtype != torch.int8:
        raise LsdError(LSD_ERR_INVALID, "d_grid must be a CUDA int8 tensor")
    if d_grid.device.index != int(device):
        raise LsdError(LSD_ERR_INVALID, "d_grid is on cuda:%d, the context on device %d" % (d_grid.device.index, int(device)))
    if cols <= 0 or rows <= 0 or tuple(d_grid.shape) not in ((rows * cols,), (rows, cols)):
        raise LsdError(LSD_ERR_INVALID, "d_grid must hold oriMapRow x oriMapCol cells, flat or [rows, cols]")
    return d_grid.contiguous()


class GridMapper:
    """Mapping with known poses: localised scans integrated into an occupancy grid on the device (k_gridmap.hip; include/lsd_hip.h,
    "mapping with known poses").  The reference has no counterpart -- its maps come from an outside SLAM --, and this is
    no full SLAM either: a pose is entered as it is (PoseGraph closes loops and rerender_device draws the grid again from the moved poses) unless the match_* methods below correct it first (locate_* finds one without a prior).  The mapper owns two planes of rows x cols counters
    (torch tensors: uint32 values in int32 storage): `pass`, the beams that crossed a cell, and `hit`, those that ended in it.  A scan at
    pose (x, y in pixels of THIS grid, ang in degrees) adds one ray per beam, cut at range_max (metres; a cut beam passes and does not
    hit); publish_device() turns the planes into the int8 OccupancyGrid (-1 below min_pass passes, 100 where hit / pass >= occ[0] /
    occ[1], else 0; the defaults are Karto's) that Localizer.set_map_device takes.  Poses from a Localizer are in pixels of the map it
    localises on: give the mapper that map's mapResol, mapOriX and mapOriY (cols and rows may differ; cells outside are skipped).
    Everything but counts() and integrate() is enqueued without waiting for the device."""

    def __init__(self, cols, rows, mapResol, mapOriX, mapOriY, range_max, min_pass=2, occ=(1, 10), ctx=None):
        import torch
        self.ctx = ctx or default_context()
        self.cols, self.rows = int(cols), int(rows)
        self.mapResol, self.mapOriX, self.mapOriY, self.range_max = float(mapResol), float(mapOriX), float(mapOriY), float(range_max)
        if not (0 < self.cols <= 65535 and 0 < self.rows <= 65535):
            raise LsdError(LSD_ERR_INVALID, "cols and rows must be 1..65535")
        if not (self.mapResol > 0 and self.range_max > 0 and self.range_max / self.mapResol < 32767):
            raise LsdError(LSD_ERR_INVALID, "mapResol > 0, range_max > 0 and range_max / mapResol < 32767")
        self.min_pass, self.occ_num, self.occ_den = _u32s(min_pass, occ[0], occ[1], limit=(1 << 32,) * 3)
        if self.occ_den == 0 or self.occ_num > self.occ_den:
            raise LsdError(LSD_ERR_INVALID, "occ = (num, den) with den > 0 and num <= den")
        self._planes = torch.zeros((2, self.rows * self.cols), dtype=torch.int32, device="cuda:%d" % int(self.ctx.device))
        self._corr = torch.zeros((self.rows, self.cols), dtype=torch.uint8, device=self._planes.device)     # likelihood_device's plane
        self._coarse = {}                                                    # coarse_device's planes, by block size
        self._pyramids = {}                                                  # pyramid_device's buffers, by the number of levels

    @property
    def map_param(self):
        """(oriMapCol, oriMapRow, mapResol, mapOriX, mapOriY) of the grid: what set_map_device takes with a published grid."""
        return (self.cols, self.rows, self.mapResol, self.mapOriX, self.mapOriY)

    @property
    def d_pass(self):
        return self._planes[0].data_ptr()

    @property
    def d_hit(self):
        return self._planes[1].data_ptr()

    def clear(self, stream=None):
        """Both planes to zero, on `stream` (a torch.cuda.Stream; default: the current one)."""
        import torch
        with torch.cuda.stream(_cuda_stream(stream)):
            self._planes.zero_()

    def _enqueue(self, ctx, d_scans, d_lens, n, stride, d_poses, pose_pitch, stream):
        ctx.enqueue_grid_integrate_device(d_scans, d_lens, n, stride, d_poses, pose_pitch, self.map_param, self.range_max, self.d_pass,
                                          self.d_hit, stream)

    def integrate_device(self, d_scans, d_lens, d_poses, pose_pitch=24, stream=None):
        """Adds scans that are on the device: d_scans a CUDA float64 tensor [n, stride, 2] as the ingest entries write it, d_lens CUDA
        int32 [n], d_poses a CUDA tensor holding n records at pose_pitch bytes, each starting with (x, y, ang) as doubles -- float64
        [n, 3] (pitch 24), or the bytes of lsd_fa_state (720) or lsd_fa_carry (768) records.  On `stream` (default: the current one)."""
        n, pitch = self._checked(d_scans, d_lens, d_poses, pose_pitch)
        self._enqueue(self.ctx, d_scans.data_ptr(), d_lens.data_ptr(), n, d_scans.shape[1], d_poses.data_ptr(), pitch,
                      _cuda_stream(stream).cuda_stream)
        self._held = (d_scans, d_lens, d_poses)                              # the launch reads them: alive until the next one

    def integrate(self, scans, lens, poses):
        """integrate_device for host arrays: scans float64 [n, stride, 2], lens int32 [n], poses float64 [n, 3]; one upload, then the
        launch on the current stream."""
        import torch
        sc, ln, po, ok = _host_scans(scans, lens, poses)
        if not ok or ((ln < 0) | (ln > sc.shape[1])).any():
            raise LsdError(LSD_ERR_INVALID, "scans [n, stride, 2], lens [n] within 0..stride, poses [n, 3]")
        dev = self._planes.device
        self.integrate_device(torch.from_numpy(sc).to(dev), torch.from_numpy(ln).to(dev), torch.from_numpy(po).to(dev))

    def publish_device(self, stream=None):
        """The planes as an OccupancyGrid: a new CUDA int8 tensor [rows, cols], written on `stream` (default: the current one) -- what
        Localizer.set_map_device(grid, *mapper.map_param) takes, on the same stream, without the host in between."""
        import torch
        ts = _cuda_stream(stream)
        with torch.cuda.stream(ts):
            grid = torch.empty((self.rows, self.cols), dtype=torch.int8, device=self._planes.device)
        self.ctx.enqueue_grid_publish_device(self.d_pass, self.d_hit, self.rows * self.cols, grid.data_ptr(), self.min_pass, self.occ_num,
                                             self.occ_den, ts.cuda_stream)
        return grid

    # -- ray casting on the grid (k_gridray.hip) --
    def _enqueue_raycast(self, ctx, d_scans, d_lens, n, stride, d_poses, pose_pitch, ray, d_grid, screened, ts):
        """(rays: a new CUDA uint8 tensor [n, stride, 32]; sums: [n, 64]; the screened scans: a new float64 tensor [n, stride, 2], or None;
        the grid that was read) of the scans at device addresses on the stream ts.  d_grid None: the mapper's own planes are published
        first, on ts."""
        import torch
        par = grid_ray(ray, mapResol=self.mapResol)
        grid = self.publish_device(ts) if d_grid is None else _occupancy_grid(d_grid, self.cols, self.rows, self.ctx.device)
        with torch.cuda.stream(ts):
            rays = torch.empty((n, stride, GRID_RAY_DTYPE.itemsize), dtype=torch.uint8, device=self._planes.device)
            sums = torch.empty((n, GRID_RAY_SUM_DTYPE.itemsize), dtype=torch.uint8, device=self._planes.device)
            so = torch.empty((n, stride, 2), dtype=torch.float64, device=self._planes.device) if screened else None
        ctx.enqueue_grid_raycast_device(d_scans, d_lens, n, stride, d_poses, pose_pitch, self.map_param, self.range_max, grid.data_ptr(), par,
                                        rays.data_ptr(), sums.data_ptr(), so.data_ptr() if screened else None, ts.cuda_stream)
        return rays, sums, so, grid

    def raycast_device(self, d_scans, d_lens, d_poses, pose_pitch=24, ray=None, d_grid=None, screened=False, stream=None):
        """Casts scans that are on the device (the arguments of integrate_device) through an int8 OccupancyGrid of the mapper's frame:
        d_grid, a CUDA int8 tensor of rows x cols cells (an outside SLAM's map serves as well), or None: the mapper's own planes, published
        first on the same stream.  ray: grid_ray() (None: its defaults; tol=None: two cells).  Returns (rays, sums): CUDA uint8 tensors
        [n, stride, 32] (GRID_RAY_DTYPE; the slots at i < len are written) and [n, 64] (GRID_RAY_SUM_DTYPE; their heads are poses:
        integrate_device(d_scans, d_lens, sums, 64) enters the scans there, a gated scan not at all); with screened also the screened
        scans, a CUDA float64 tensor [n, stride, 2].  On `stream`; nothing waits."""
        n, pitch = self._checked(d_scans, d_lens, d_poses, pose_pitch)
        rays, sums, so, grid = self._enqueue_raycast(self.ctx, d_scans.data_ptr(), d_lens.data_ptr(), n, d_scans.shape[1], d_poses.data_ptr(), pitch,
                                                     ray, d_grid, screened, _cuda_stream(stream))
        self._held_ray = (d_scans, d_lens, d_poses, grid)                    # the launches read them: alive until the next call
        return (rays, sums, so) if screened else (rays, sums)

    def raycast(self, scans, lens, poses, ray=None, grid=None):
        """raycast_device for host arrays (scans float64 [n, stride, 2], lens int32 [n], poses float64 [n, 3]; grid: int8 [rows, cols], or
        None: the mapper's own).  Returns (rays GRID_RAY_DTYPE [n, stride], sums GRID_RAY_SUM_DTYPE [n]) as numpy arrays: a read-back,
        which waits for the device.  The record slots at i >= len are zero."""
        import torch
        sc, ln, po, ok = _host_scans(scans, lens, poses)
        if not ok or ((ln < 0) | (ln > sc.shape[1])).any():
            raise LsdError(LSD_ERR_INVALID, "scans [n, stride, 2], lens [n] within 0..stride, poses [n, 3]")
        dev = self._planes.device
        d_grid = None if grid is None else torch.from_numpy(np.ascontiguousarray(grid, np.int8)).to(dev)
        rays, sums = self.raycast_device(torch.from_numpy(sc).to(dev), torch.from_numpy(ln).to(dev), torch.from_numpy(po).to(dev), 24, ray, d_grid)
        out = rays.cpu().numpy().reshape(-1).view(GRID_RAY_DTYPE).reshape(sc.shape[:2]).copy()
        out[np.arange(sc.shape[1])[None, :] >= ln[:, None]] = np.zeros((), GRID_RAY_DTYPE)
        return out, sums.cpu().numpy().reshape(-1).view(GRID_RAY_SUM_DTYPE).copy()

    def _screen_and_integrate(self, ctx, d_scans, d_lens, n, stride, d_poses, pose_pitch, ray, d_grid, ts):
        rays, sums, so, grid = self._enqueue_raycast(ctx, d_scans, d_lens, n, stride, d_poses, pose_pitch, ray, d_grid, True, ts)
        self._enqueue(ctx, so.data_ptr(), d_lens, n, stride, sums.data_ptr(), GRID_RAY_SUM_DTYPE.itemsize, ts.cuda_stream)
        self._held_screen = (rays, sums, so, grid)
        return rays, sums

    @property
    def last_screened(self):
        """The screened scans the last screen_and_integrate_device / screen_and_integrate_last_tick integrated: a CUDA float64 tensor
        [n, stride, 2] (the readings at i < len are written), or None before the first."""
        held = getattr(self, "_held_screen", None)
        return held[2] if held else None

    def screen_and_integrate_device(self, d_scans, d_lens, d_poses, pose_pitch=24, ray=None, d_grid=None, stream=None):
        """Integration with the ray-casting stage in front, in stream order: the grid (d_grid, or None: the mapper's own planes published
        now) is read by raycast_device with screened scans, and the screened scans are integrated at the summary records (pitch 64) -- the
        readings of the classes grid_ray(drop=) names are gone, and with gate a scan that does not agree with the map adds nothing.
        Every scan of the call is judged against the grid as it was before the call.  Returns (rays, sums); nothing waits."""
        n, pitch = self._checked(d_scans, d_lens, d_poses, pose_pitch)
        got = self._screen_and_integrate(self.ctx, d_scans.data_ptr(), d_lens.data_ptr(), n, d_scans.shape[1], d_poses.data_ptr(), pitch, ray,
                                         d_grid, _cuda_stream(stream))
        self._held_ray = (d_scans, d_lens, d_poses)
        return got

    # -- correlative scan-to-grid matching (k_gridmatch.hip) --
    @property
    def d_corr(self):
        return self._corr.data_ptr()

    def likelihood_device(self, smear=None, stream=None, block=0):
        """Refreshes the mapper's lookup plane from its counters, on `stream` (default: the current one): every occupied cell (what
        publish_device gives 100) smeared by `smear` (default: grid_smear_default(1.0, 3)).  Returns the plane, a CUDA uint8 tensor
        [rows, cols] the mapper owns.  block = 2..16: coarse_device(block) behind it."""
        self.ctx.enqueue_grid_likelihood_device(self.d_pass, self.d_hit, self.cols, self.rows, self.d_corr, self.min_pass, self.occ_num,
                                                self.occ_den, smear, _cuda_stream(stream).cuda_stream)
        if block:
            self.coarse_device(block, stream)
        return self._corr

    def coarse_device(self, block, stream=None):
        """Refreshes the plane of block maxima of the lookup plane as it is now (k_gridmatch_mr.hip), on `stream` (default:
        the current one).  block: 2..16.  Returns the plane, a CUDA uint8 tensor [rows + block - 1, cols + block - 1] the mapper owns (one
        per block size, allocated at its first use)."""
        import torch
        b = int(block)
        if not 2 <= b <= 16:
            raise LsdError(LSD_ERR_INVALID, "block must be 2..16")
        ts = _cuda_stream(stream)
        if b not in self._coarse:
            with torch.cuda.stream(ts):
                self._coarse[b] = torch.zeros((self.rows + b - 1, self.cols + b - 1), dtype=torch.uint8, device=self._planes.device)
        self.ctx.enqueue_grid_coarse_device(self.d_corr, self.cols, self.rows, b, self._coarse[b].data_ptr(), ts.cuda_stream)
        return self._coarse[b]

    def _enqueue_match(self, ctx, d_scans, d_lens, n, stride, d_poses, pose_pitch, search, ts, block=0, stats=False):
        """n records (a new CUDA uint8 tensor [n, 56]) of the scans at device addresses, matched on the mapper's plane on the stream ts.
        block: 0 the plain search, 2..16 the coarse-to-fine one on the coarse plane coarse_device(block) wrote last; with stats (records, a
        new CUDA uint8 tensor [n, 16])."""
        import torch
        with torch.cuda.stream(ts):
            rec = torch.empty((n, GRID_MATCH_DTYPE.itemsize), dtype=torch.uint8, device=self._planes.device)
        if not block:
            if stats:
                raise LsdError(LSD_ERR_INVALID, "stats come with block = 2..16")
            ctx.enqueue_grid_match_device(d_scans, d_lens, n, stride, d_poses, pose_pitch, self.map_param, self.range_max, self.d_corr, search,
                                          rec.data_ptr(), ts.cuda_stream)
            return rec
        b = int(block)
        if b not in self._coarse:
            self.coarse_device(b, ts)
        st = None
        if stats:
            with torch.cuda.stream(ts):
                st = torch.empty((n, GRID_MATCH_MR_STATS_DTYPE.itemsize), dtype=torch.uint8, device=self._planes.device)
        ctx.enqueue_grid_match_mr_device(d_scans, d_lens, n, stride, d_poses, pose_pitch, self.map_param, self.range_max, self.d_corr,
                                         self._coarse[b].data_ptr(), b, search, rec.data_ptr(), st.data_ptr() if stats else None, ts.cuda_stream)
        return (rec, st) if stats else rec

    def _checked_scans(self, d_scans, d_lens):
        import torch
        for name, t, dt in (("d_scans", d_scans, torch.float64), ("d_lens", d_lens, torch.int32)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dt or not t.is_contiguous():
                raise LsdError(LSD_ERR_INVALID, "%s must be a contiguous CUDA %s tensor" % (name, str(dt).replace("torch.", "")))
        n = d_lens.numel()
        if d_scans.dim() != 3 or d_scans.shape[0] != n or d_scans.shape[2] != 2 or d_scans.shape[1] < 1:
            raise LsdError(LSD_ERR_INVALID, "d_scans must be [n, stride >= 1, 2] with one length per scan")
        return n

    def _checked(self, d_scans, d_lens, d_poses, pose_pitch):
        import torch
        n, pitch = self._checked_scans(d_scans, d_lens), int(pose_pitch)
        if not isinstance(d_poses, torch.Tensor) or not d_poses.is_cuda or not d_poses.is_contiguous():
            raise LsdError(LSD_ERR_INVALID, "d_poses must be a contiguous CUDA tensor")
        if pitch < 24 or (n and d_poses.numel() * d_poses.element_size() < (n - 1) * pitch + 24):
            raise LsdError(LSD_ERR_INVALID, "d_poses holds fewer than n records of pose_pitch >= 24 bytes")
        return n, pitch

    def _enqueue_response(self, ctx, d_scans, d_lens, n, stride, d_poses, pose_pitch, d_records, search, response, ts, volume=False):
        """n response records (a new CUDA uint8 tensor [n, 192]) of the scans at device addresses, from the match records at d_records and
        the ORIGINAL poses at d_poses, on the mapper's plane on the stream ts; ang_step is `search`'s.  With volume (records, the scores: a
        new CUDA int32 tensor [n, 2 ra + 1, 2 ry + 1, 2 rx + 1] holding uint32 values)."""
        import torch
        rp, se = grid_response(response), grid_search(search)
        with torch.cuda.stream(ts):
            out = torch.empty((n, GRID_RESPONSE_DTYPE.itemsize), dtype=torch.uint8, device=self._planes.device)
            vol = torch.empty((n, 2 * rp.ra + 1, 2 * rp.ry + 1, 2 * rp.rx + 1), dtype=torch.int32, device=self._planes.device) if volume else None
        ctx.enqueue_grid_response_device(d_scans, d_lens, n, stride, d_poses, pose_pitch, d_records, self.map_param, self.range_max, self.d_corr,
                                         se.ang_step, rp, out.data_ptr(), vol.data_ptr() if volume else None, ts.cuda_stream)
        return (out, vol) if volume else out

    def response_device(self, d_scans, d_lens, d_poses, d_records, pose_pitch=24, search=None, response=None, stream=None, volume=False):
        """The response around a match (k_gridresponse.hip): for the scans and the ORIGINAL poses match_device was given
        and the records it returned (either search wrote them), the scores in the neighbourhood `response` (grid_response(); None: its
        defaults) of each winner, on the plane likelihood_device wrote last; `search` is the match's (its ang_step is read).  Returns the
        response records: a CUDA uint8 tensor [n, 192] (GRID_RESPONSE_DTYPE) whose heads are the refined poses --
        integrate_device(d_scans, d_lens, responses, 192) enters the scans there --, with a covariance, the sub-cell offsets and the integer
        moments behind them.  volume=True: (records, the scores).  On `stream`; nothing waits."""
        import torch
        n, pitch = self._checked(d_scans, d_lens, d_poses, pose_pitch)
        if (not isinstance(d_records, torch.Tensor) or not d_records.is_cuda or not d_records.is_contiguous() or
                d_records.numel() * d_records.element_size() < n * GRID_MATCH_DTYPE.itemsize):
            raise LsdError(LSD_ERR_INVALID, "d_records must be a contiguous CUDA tensor of n records of 56 bytes")
        got = self._enqueue_response(self.ctx, d_scans.data_ptr(), d_lens.data_ptr(), n, d_scans.shape[1], d_poses.data_ptr(), pitch,
                                     d_records.data_ptr(), search, response, _cuda_stream(stream), volume)
        self._held_response = (d_scans, d_lens, d_poses, d_records)
        return got

    def match_device(self, d_scans, d_lens, d_poses, pose_pitch=24, search=None, stream=None, block=0, stats=False, response=None):
        """Matches scans that are on the device (the arguments of integrate_device) on the plane likelihood_device wrote last, over the
        window `search` (grid_search(); None: its defaults).  Returns the records: a CUDA uint8 tensor [n, 56] (GRID_MATCH_DTYPE), whose
        heads are the corrected poses -- integrate_device(d_scans, d_lens, records, 56) enters the scans there.  On `stream`.
        block = 2..16: the same records by the coarse-to-fine search, on the coarse plane of the last coarse_device(block) /
        likelihood_device(block=block) (made now if there is none yet); then stats=True returns (records, statistics: a CUDA uint8 tensor
        [n, 16], GRID_MATCH_MR_STATS_DTYPE).  response (grid_response(); True: its defaults) given: response_device behind the match, and
        its records are returned beside what is returned without it."""
        n, pitch = self._checked(d_scans, d_lens, d_poses, pose_pitch)
        got = self._chain(self.ctx, d_scans.data_ptr(), d_lens.data_ptr(), n, d_scans.shape[1], d_poses.data_ptr(), pitch, search,
                          _cuda_stream(stream), block, stats, response)
        self._held_match = (d_scans, d_lens, d_poses, got)
        return got

    def match(self, scans, lens, poses, search=None, block=0, response=None):
        """match_device for host arrays (scans float64 [n, stride, 2], lens int32 [n], poses float64 [n, 3]); returns the records as a numpy
        array of GRID_MATCH_DTYPE: a read-back, which waits for the device.  response given: (records, the response records as a numpy
        array of GRID_RESPONSE_DTYPE)."""
        import torch
        sc, ln, po, ok = _host_scans(scans, lens, poses)
        if not ok or ((ln < 0) | (ln > sc.shape[1])).any():
            raise LsdError(LSD_ERR_INVALID, "scans [n, stride, 2], lens [n] within 0..stride, poses [n, 3]")
        dev = self._planes.device
        rec = self.match_device(torch.from_numpy(sc).to(dev), torch.from_numpy(ln).to(dev), torch.from_numpy(po).to(dev), 24, search, block=block,
                                response=response)
        if response is None:
            return rec.cpu().numpy().reshape(-1).view(GRID_MATCH_DTYPE).copy()
        return (rec[0].cpu().numpy().reshape(-1).view(GRID_MATCH_DTYPE).copy(), rec[1].cpu().numpy().reshape(-1).view(GRID_RESPONSE_DTYPE).copy())

    def _chain(self, ctx, d_scans, d_lens, n, stride, d_poses, pose_pitch, search, ts, block=0, stats=False, response=None, integrate=False,
               refresh=False, smear=None, integrate_at="match"):
        """What match_device, match_and_integrate_device and Localizer.refine_and_integrate_last_tick enqueue on the stream ts, in this
        order: likelihood_device (refresh), the match (block: coarse to fine), the response (response given) and, with integrate, the
        integration at the match records or at the response's.  Returns the records, with the statistics (stats) and then the response
        records (response given) behind them in a tuple."""
        if integrate and (integrate_at not in ("match", "response") or (integrate_at == "response" and response is None)):
            raise LsdError(LSD_ERR_INVALID, "integrate_at is 'match' or, with response given, 'response'")
        if refresh:
            self.likelihood_device(smear, ts, block)
        got = self._enqueue_match(ctx, d_scans, d_lens, n, stride, d_poses, pose_pitch, search, ts, block, stats)
        parts = list(got) if stats else [got]
        if response is not None:
            parts.append(self._enqueue_response(ctx, d_scans, d_lens, n, stride, d_poses, pose_pitch, parts[0].data_ptr(), search, response, ts))
        got = tuple(parts) if len(parts) > 1 else parts[0]
        if integrate:
            at = parts[-1] if integrate_at == "response" else parts[0]      # records of 192 or of 56 bytes, a pose at the head of each
            self._enqueue(ctx, d_scans, d_lens, n, stride, at.data_ptr(), at.shape[1], ts.cuda_stream)
            self._held_rec = got                                             # the integration reads it: alive until the next one
        return got

    def match_and_integrate_device(self, d_scans, d_lens, d_poses, pose_pitch=24, search=None, stream=None, refresh=True, smear=None, block=0,
                                   stats=False, response=None, integrate_at="match"):
        """In stream order: likelihood_device(smear) (refresh=False: the plane as it is), match_device, then integrate_device at the records
        (pitch 56).  All scans of one call are matched against the plane as it was before the call.  Returns the records.  block = 2..16:
        the coarse-to-fine search -- the coarse plane is refreshed whenever the lookup plane is --, and stats=True returns (records,
        statistics) as match_device does.  response given: response_device behind the match, its records returned beside the others; then
        integrate_at="response" integrates at the refined poses (pitch 192) instead of the records' ("match", the default)."""
        n, pitch = self._checked(d_scans, d_lens, d_poses, pose_pitch)
        rec = self._chain(self.ctx, d_scans.data_ptr(), d_lens.data_ptr(), n, d_scans.shape[1], d_poses.data_ptr(), pitch, search,
                          _cuda_stream(stream), block, stats, response, integrate=True, refresh=refresh, smear=smear, integrate_at=integrate_at)
        self._held_match = (d_scans, d_lens, d_poses)
        return rec

    # -- global scan-to-grid localisation (k_gridlocate.hip) --
    def pyramid_device(self, levels, stream=None):
        """Refreshes the pyramid of block maxima of the lookup plane as it is now, levels 0..levels, on `stream` (default: the current
        one).  Returns the buffer, a CUDA uint8 tensor of grid_pyramid_bytes(cols, rows, levels) bytes the mapper owns (one per number of
        levels, allocated at its first use); level h starts at grid_pyramid_offset(cols, rows, h)."""
        import torch
        H = int(levels)
        if not 0 <= H <= GRID_LOCATE_MAX_LEVELS:
            raise LsdError(LSD_ERR_INVALID, "levels must be 0..8")
        ts = _cuda_stream(stream)
        pyr = self._pyramids
        if H not in pyr:
            with torch.cuda.stream(ts):
                pyr[H] = torch.zeros(grid_pyramid_bytes(self.cols, self.rows, H), dtype=torch.uint8, device=self._planes.device)
        self.ctx.enqueue_grid_pyramid_device(self.d_corr, self.cols, self.rows, H, pyr[H].data_ptr(), ts.cuda_stream)
        return pyr[H]

    def _enqueue_locate(self, ctx, d_scans, d_lens, n, stride, locate, refresh, smear, stats, ts, tight=None):
        """In stream order on ts: likelihood_device(smear) (refresh), pyramid_device, the location of the scans at device addresses.  n
        records (a new CUDA uint8 tensor [n, 64]); with stats (records, a new CUDA uint8 tensor [n, 48]).  tight (grid_locate_tight())
        other than None / 0 / False: the tight entry, whose statistics are [n, 128]."""
        import torch
        par = grid_locate(locate, cols=self.cols, rows=self.rows)
        word = grid_locate_tight(tight)
        if refresh:
            self.likelihood_device(smear, ts)
        pyr = self.pyramid_device(par.levels, ts)
        with torch.cuda.stream(ts):
            rec = torch.empty((n, GRID_LOCATE_DTYPE.itemsize), dtype=torch.uint8, device=self._planes.device)
            width = (GRID_LOCATE_TIGHT_STATS_DTYPE if word else GRID_LOCATE_STATS_DTYPE).itemsize
            st = torch.empty((n, width), dtype=torch.uint8, device=self._planes.device) if stats else None
        if word:
            ctx.enqueue_grid_locate_tight_device(d_scans, d_lens, n, stride, self.map_param, self.range_max, pyr.data_ptr(), par, word, rec.data_ptr(),
                                                 st.data_ptr() if stats else None, ts.cuda_stream)
        else:
            ctx.enqueue_grid_locate_device(d_scans, d_lens, n, stride, self.map_param, self.range_max, pyr.data_ptr(), par, rec.data_ptr(),
                                           st.data_ptr() if stats else None, ts.cuda_stream)
        return (rec, st) if stats else rec

    def locate_device(self, d_scans, d_lens, locate=None, refresh=True, smear=None, stats=False, stream=None, tight=None):
        """Locates scans that are on the device (d_scans, d_lens of integrate_device) on the mapper's grid WITHOUT a prior pose: in stream
        order likelihood_device(smear) (refresh=False: the plane as it is), pyramid_device and the search over the box and the headings of
        `locate` (grid_locate(); None: the whole grid, its placeholder defaults).  Returns the records: a CUDA uint8 tensor [n, 64]
        (GRID_LOCATE_DTYPE) whose heads are poses -- the located one where flags is GRID_LOCATE_ACCEPTED, else the "no pose" sentinel, so
        match_device(d_scans, d_lens, records, 64) and integrate_device(d_scans, d_lens, records, 64) take them and skip the rest.
        n_best > 1 says the map is ambiguous.  stats=True: (records, statistics: a CUDA uint8 tensor [n, 48], GRID_LOCATE_STATS_DTYPE).
        tight (None, 0, False: this search as it is; True, "probe", "retry" or a flag word: grid_locate_tight()): the bound raised level by
        level and a level that overflows retried once -- the same records wherever neither search overflows, fewer
        overflows; the statistics are then [n, 128], GRID_LOCATE_TIGHT_STATS_DTYPE.  On `stream`; nothing waits."""
        n = self._checked_scans(d_scans, d_lens)
        got = self._enqueue_locate(self.ctx, d_scans.data_ptr(), d_lens.data_ptr(), n, d_scans.shape[1], locate, refresh, smear, stats,
                                   _cuda_stream(stream), tight)
        self._held_locate = (d_scans, d_lens)                                # the launches read them: alive until the next call
        return got

    def locate(self, scans, lens, locate=None, refresh=True, smear=None, stats=False, tight=None):
        """locate_device for host arrays (scans float64 [n, stride, 2], lens int32 [n]); returns the records as a numpy array of
        GRID_LOCATE_DTYPE (stats=True: with the statistics as GRID_LOCATE_STATS_DTYPE, under `tight` GRID_LOCATE_TIGHT_STATS_DTYPE): a
        read-back, which waits for the device."""
        import torch
        ln0 = np.atleast_1d(np.asarray(lens))
        sc, ln, _, ok = _host_scans(scans, lens, np.zeros((len(ln0), 3)))
        if not ok or ((ln < 0) | (ln > sc.shape[1])).any():
            raise LsdError(LSD_ERR_INVALID, "scans [n, stride, 2], lens [n] within 0..stride")
        dev = self._planes.device
        got = self.locate_device(torch.from_numpy(sc).to(dev), torch.from_numpy(ln).to(dev), locate, refresh, smear, stats, tight=tight)
        if not stats:
            return got.cpu().numpy().reshape(-1).view(GRID_LOCATE_DTYPE).copy()
        st_dtype = GRID_LOCATE_TIGHT_STATS_DTYPE if grid_locate_tight(tight) else GRID_LOCATE_STATS_DTYPE
        return got[0].cpu().numpy().reshape(-1).view(GRID_LOCATE_DTYPE).copy(), got[1].cpu().numpy().reshape(-1).view(st_dtype).copy()

    def counts(self):
        """(pass, hit) as numpy uint32 [rows, cols]: a read-back, which waits for the device."""
        both = self._planes.cpu().numpy().view(np.uint32).reshape(2, self.rows, self.cols)
        return both[0].copy(), both[1].copy()

    def rerender_device(self, graph, stream=None):
        """The grid drawn again from a PoseGraph's nodes as they are now: clear(), then the graph's WHOLE keyframe
        store integrated at its nodes (pitch 64) -- the rows past n_nodes have length 0 and fall out as empty scans, so the host does
        not need n_nodes.  On `stream` (default: the current one); nothing waits."""
        if not isinstance(graph, PoseGraph):
            raise LsdError(LSD_ERR_INVALID, "graph must be a PoseGraph")
        ts = _cuda_stream(stream)
        self.clear(ts)
        self._enqueue(graph.ctx, graph._store.data_ptr(), graph._store_lens.data_ptr(), graph.nodes_cap, graph.n_beams, graph._nodes.data_ptr(),
                      PG_NODE_DTYPE.itemsize, ts.cuda_stream)


class PoseGraph:
    """A pose graph on the device (k_pgbuild.hip, k_posegraph.hip; include/lsd_hip.h, "pose graph"): keyframes with
    their scans, odometry edges between neighbours of a track, closure edges from a scan matched against the neighbourhood of an old node,
    and the relaxation that redistributes the error; GridMapper.rerender_device(graph) then draws the grid again from the moved poses.
    The graph owns head, nodes, edges, tracks, the keyframe store and the workspace as torch tensors; the counts live on the device.
    optimize_device() makes the relaxation robust against closures that are confidently wrong and takes them out on the device (DESIGN.md
    8.1.16); close_place_device() finds the anchor of a closure by the appearance of the scan where the drift has carried the pose out of
    close_device()'s radius; close_all_device() asks that of every keyframe in one launch and closes every distinct
    loop it finds; relax_device() and optimize_device() take precond="chain" for long tracks, and
    reduce_device() retires redundant keyframes and compacts the graph, so that it stops growing where a robot patrols (DESIGN.md
    8.1.21); the workspace has that preconditioner's size from the construction on -- 432 bytes per node of nodes_cap more than the default one
    needs, whether precond is ever used or not --, so that no enqueue allocates.  Everything but nodes(), edges(), node_map(), place_records(), loop_records(), the *report() and *reports()
    methods and disable_edges() is enqueued without waiting for the device."""

    def __init__(self, nodes_cap, edges_cap, n_beams, n_tracks=1, ctx=None):
        import torch
        self.ctx = ctx or default_context()
        self.nodes_cap, self.edges_cap, self.n_beams, self.n_tracks = int(nodes_cap), int(edges_cap), int(n_beams), int(n_tracks)
        ws = pg_workspace_bytes(self.nodes_cap, self.edges_cap)
        if ws == 0 or self.n_beams < 1 or self.n_tracks < 1:
            raise LsdError(LSD_ERR_INVALID, "nodes_cap 1..16384, edges_cap 1..65536, n_beams >= 1, n_tracks >= 1")
        dev = "cuda:%d" % int(self.ctx.device)

        def z(*shape, dtype=torch.uint8):
            return torch.zeros(shape, dtype=dtype, device=dev)
        self._head, self._nodes, self._edges = z(PG_HEAD_DTYPE.itemsize), z(self.nodes_cap, PG_NODE_DTYPE.itemsize), z(self.edges_cap, PG_EDGE_DTYPE.itemsize)
        tracks = np.zeros(self.n_tracks, PG_TRACK_DTYPE)
        tracks["last"] = -1
        self._tracks = torch.from_numpy(tracks.view(np.uint8).reshape(self.n_tracks, -1)).to(dev)
        self._store, self._store_lens = z(self.nodes_cap, self.n_beams, 2, dtype=torch.float64), z(self.nodes_cap, dtype=torch.int32)
        self._ws = z(max(ws, pg_workspace_pc_bytes(self.nodes_cap, self.edges_cap, "chain")))      # (the larger of the two preconditioners')
        self._append_rep, self._near, self._closure_rep = z(PG_APPEND_REP_DTYPE.itemsize), z(PG_NEAR_DTYPE.itemsize), z(PG_CLOSURE_REP_DTYPE.itemsize)
        self._relax_rep = z(PG_RELAX_REP_DTYPE.itemsize)
        self._robust_rep, self._prune_rep = z(PG_ROBUST_REP_DTYPE.itemsize), z(PG_PRUNE_REP_DTYPE.itemsize)
        self._precond_rep = z(PG_PRECOND_REP_DTYPE.itemsize)
        self._sel = z(self.nodes_cap, 3, dtype=torch.float64)
        self._q_scan, self._q_len, self._q_pose = z(1, self.n_beams, 2, dtype=torch.float64), z(1, dtype=torch.int32), z(1, 3, dtype=torch.float64)
        # place recognition: zeroed descriptors are "not described yet"
        self._desc, self._place_work = z(self.nodes_cap, PG_DESC_DTYPE.itemsize), z(self.nodes_cap, dtype=torch.int32)
        self._place_recs, self._place_rep = z(PG_PLACE_MAX, PG_PLACE_REC_DTYPE.itemsize), z(PG_PLACE_REP_DTYPE.itemsize)
        self._desc_range_max = None
        # every loop of a track: the batch's records, the loops, and per loop what a closure attempt leaves
        self._all_recs, self._all_reps = z(self.nodes_cap * PG_PLACE_MAX, PG_PLACE_REC_DTYPE.itemsize), z(self.nodes_cap, PG_PLACE_REP_DTYPE.itemsize)
        self._loops_ws = z(pg_loops_workspace_bytes(self.nodes_cap, PG_PLACE_MAX, self.edges_cap))
        self._loops, self._loops_rep = z(PG_LOOPS_MAX, PG_LOOP_REC_DTYPE.itemsize), z(PG_LOOPS_REP_DTYPE.itemsize)
        self._loop_near, self._loop_closure_rep = z(PG_LOOPS_MAX, PG_NEAR_DTYPE.itemsize), z(PG_LOOPS_MAX, PG_CLOSURE_REP_DTYPE.itemsize)
        self._all_q = None                                                   # (q_lo, n_q, k, gap, window) of the last recognize_all_device
        self._loops_max = 0                                                  # max_loops of the last find_loops_device
        # marginal covariances and the gate: the copy of the head, the queries "every node" and "new edge k", one report;
        # the records and the workspace get their size with the first call that needs it (slots slices of vectors: marginals_device)
        self._prior, self._marg_rep = z(PG_HEAD_DTYPE.itemsize), z(PG_MARG_REP_DTYPE.itemsize)
        every = np.zeros(max(self.nodes_cap, PG_LOOPS_MAX), PG_MARG_QUERY_DTYPE)
        every["a"] = np.arange(len(every))
        new = every[:PG_LOOPS_MAX].copy()
        new["kind"] = PG_MARG_NEW_EDGE
        self._q_every, self._q_new = (torch.from_numpy(q.view(np.int32).reshape(len(q), 4)).to(dev) for q in (every[:self.nodes_cap], new))
        self._marg_q, self._marg_n, self._marg_every, self._marg_recs, self._vet_reps, self._marg_ws = None, 0, False, None, None, None
        # reduce: the map, the report and a workspace of its own, sized here so that no enqueue allocates
        self._map, self._reduce_rep = z(self.nodes_cap, dtype=torch.int32), z(PG_REDUCE_REP_DTYPE.itemsize)
        self._reduce_ws = z(max(pg_reduce_workspace_bytes(self.nodes_cap, self.edges_cap, self.n_beams), 16))

    def _track(self, track):
        t = int(track)
        if not 0 <= t < self.n_tracks:
            raise LsdError(LSD_ERR_INVALID, "track must be 0..%d" % (self.n_tracks - 1))
        return t, self._tracks.data_ptr() + t * PG_TRACK_DTYPE.itemsize

    def _store_args(self):
        """The store as every entry takes it: the rows, their lengths, the stride."""
        return self._store.data_ptr(), self._store_lens.data_ptr(), self.n_beams

    def _hand_over(self, d_near=None):
        """What near, recognize and loop_select leave for _close_tail: the near record (the graph's own, or d_near), the selection, the
        one-row batch, its length and its pose."""
        return d_near or self._near.data_ptr(), self._sel.data_ptr(), self._q_scan.data_ptr(), self._q_len.data_ptr(), self._q_pose.data_ptr()

    @staticmethod
    def _scratch(scratch_mapper):
        if not isinstance(scratch_mapper, GridMapper):
            raise LsdError(LSD_ERR_INVALID, "scratch_mapper must be a GridMapper")

    def _append(self, d_scans, d_lens, n, stride, d_poses, pose_pitch, track, append, ts):
        t, d_track = self._track(track)
        self.ctx.enqueue_pg_append_device(d_scans, d_lens, n, stride, d_poses, pose_pitch, self._head.data_ptr(), self._nodes.data_ptr(),
                                          self.nodes_cap, self._edges.data_ptr(), self.edges_cap, d_track, t, *self._store_args(), append,
                                          self._append_rep.data_ptr(), ts.cuda_stream)

    def append_device(self, d_scans, d_lens, d_poses, pose_pitch=24, track=0, append=None, stream=None):
        """Candidate frames that are on the device (the arguments of GridMapper.integrate_device), in order, against `track`: a frame
        min_dist pixels or min_ang degrees from the track's last keyframe (pg_append()) becomes a node, its scan a row of the store,
        the measured motion an edge.  Node 0 is appended fixed.  On `stream` (default: the current one)."""
        import torch
        for name, t, dt in (("d_scans", d_scans, torch.float64), ("d_lens", d_lens, torch.int32)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dt or not t.is_contiguous():
                raise LsdError(LSD_ERR_INVALID, "%s must be a contiguous CUDA %s tensor" % (name, str(dt).replace("torch.", "")))
        n, pitch = d_lens.numel(), int(pose_pitch)
        if d_scans.dim() != 3 or d_scans.shape[0] != n or d_scans.shape[2] != 2 or d_scans.shape[1] < 1:
            raise LsdError(LSD_ERR_INVALID, "d_scans must be [n, stride >= 1, 2] with one length per scan")
        if (not isinstance(d_poses, torch.Tensor) or not d_poses.is_cuda or not d_poses.is_contiguous() or pitch < 24 or
                (n and d_poses.numel() * d_poses.element_size() < (n - 1) * pitch + 24)):
            raise LsdError(LSD_ERR_INVALID, "d_poses must be a contiguous CUDA tensor of n records of pose_pitch >= 24 bytes")
        self._append(d_scans.data_ptr(), d_lens.data_ptr(), n, d_scans.shape[1], d_poses.data_ptr(), pitch, track, append, _cuda_stream(stream))
        self._held = (d_scans, d_lens, d_poses)                              # the launch reads them: alive until the next one

    def near_device(self, track=0, gap=10, radius=10.0, window=2, stream=None):
        """The loop candidate of the track's last node (lsd_enqueue_pg_near_device), into the graph's own near record, selection and
        one-row batch.  On `stream`."""
        _, d_track = self._track(track)
        self.ctx.enqueue_pg_near_device(self._head.data_ptr(), self._nodes.data_ptr(), self.nodes_cap, d_track, *self._store_args(), gap, radius, window,
                                        *self._hand_over(), _cuda_stream(stream).cuda_stream)

    def close_device(self, scratch_mapper, track=0, gap=10, radius=10.0, window=2, search=None, response=None, smear=None, closure=None,
                     stream=None, vet=None):
        """One attempt at a loop closure for the last node of `track`, on one stream, in this order: near_device; scratch_mapper.clear();
        the WHOLE store integrated at the selection -- the anchor's neighbourhood alone, without the host knowing the anchor --;
        scratch_mapper.likelihood_device(smear); match plus response of the one gathered row; the closure edge.  scratch_mapper: a
        GridMapper of the map's frame that this call overwrites.  Returns the response record of the query, a CUDA uint8 tensor
        [1, 192]; closure_report() says what came of it.  vet: None, or pg_vet()'s dict(gate=, marg=): snapshot_device() in front, and
        behind the closure the marginal of the new edge's two ends on the graph without it and the gate, which takes a closure the
        graph finds implausible out again before anything is relaxed (vet_reports(), marginal_records()).  Nothing
        waits."""
        self._scratch(scratch_mapper)
        ts = _cuda_stream(stream)
        vet = None if vet is None else pg_vet(vet)
        if vet:
            self.snapshot_device(ts)
        self.near_device(track, gap, radius, window, ts)
        resp = self._close_tail(scratch_mapper, search, response, smear, closure, ts)
        if vet:
            self._vetted(vet, 1, ts)
        return resp

    def _close_tail(self, scratch_mapper, search, response, smear, closure, ts, d_near=None, d_closure_rep=None):
        """What follows the choice of an anchor, by pose (near_device) or by appearance (recognize_device, or loop m of
        close_all_device, which names its own near record and closure report): the neighbourhood drawn from the selection, the gathered
        row matched on it with its response, the closure edge."""
        scratch_mapper.clear(ts)
        scratch_mapper._enqueue(self.ctx, self._store.data_ptr(), self._store_lens.data_ptr(), self.nodes_cap, self.n_beams, self._sel.data_ptr(), 24,
                                ts.cuda_stream)
        scratch_mapper.likelihood_device(smear, ts)
        rec, resp = scratch_mapper._chain(self.ctx, self._q_scan.data_ptr(), self._q_len.data_ptr(), 1, self.n_beams, self._q_pose.data_ptr(), 24,
                                          search, ts, response=True if response is None else response)
        self.ctx.enqueue_pg_closure_device(self._head.data_ptr(), self._nodes.data_ptr(), self.nodes_cap, self._edges.data_ptr(), self.edges_cap,
                                           d_near or self._near.data_ptr(), resp.data_ptr(), closure,
                                           d_closure_rep or self._closure_rep.data_ptr(), ts.cuda_stream)
        self._held_close = (rec, resp)                                       # the launches read them: alive until the next call
        return resp

    def describe_device(self, range_max, stream=None):
        """The descriptors (lsd_enqueue_pg_describe_device) of the keyframes that have none yet; the count is read on the device, so this
        may be called after every append.  A descriptor depends on range_max: a graph keeps the first one and refuses another.  On
        `stream`; nothing waits."""
        rm = float(range_max)
        if self._desc_range_max is not None and rm != self._desc_range_max:
            raise LsdError(LSD_ERR_INVALID, "this graph's descriptors were made with range_max %r" % self._desc_range_max)
        self.ctx.enqueue_pg_describe_device(self._head.data_ptr(), self.nodes_cap, *self._store_args(), rm, self._desc.data_ptr(),
                                            _cuda_stream(stream).cuda_stream)
        self._desc_range_max = rm

    def recognize_device(self, range_max, track=0, place=None, stream=None):
        """The loop candidate of the track's last node by the appearance of its scan (describe_device, then
        lsd_enqueue_pg_recognize_device), into the graph's own near record, selection and one-row batch -- what near_device leaves, with
        the anchor's pose turned by the descriptors' shift as the query's pose.  place: pg_place().  place_records() and place_report()
        say what was found.  On `stream`; nothing waits."""
        _, d_track = self._track(track)
        ts = _cuda_stream(stream)
        par = pg_place(place)
        self.describe_device(range_max, ts)
        self.ctx.enqueue_pg_recognize_device(self._head.data_ptr(), self._nodes.data_ptr(), self.nodes_cap, d_track, *self._store_args(),
                                             self._desc.data_ptr(), par, self._place_work.data_ptr(), self._place_recs.data_ptr(),
                                             self._place_rep.data_ptr(), *self._hand_over(), ts.cuda_stream)
        self._place_k = int(par.k)

    def close_place_device(self, scratch_mapper, track=0, place=None, search=None, response=None, smear=None, closure=None, stream=None, vet=None):
        """close_device with the anchor found by recognize_device instead of near_device: a loop that odometry has NOT almost closed.
        range_max is the scratch mapper's.  Returns the response record of the query; closure_report(), place_report() and
        place_records() say what came of it.  vet: as close_device's.  Nothing waits."""
        self._scratch(scratch_mapper)
        ts = _cuda_stream(stream)
        vet = None if vet is None else pg_vet(vet)
        if vet:
            self.snapshot_device(ts)
        self.recognize_device(scratch_mapper.range_max, track, place, ts)
        resp = self._close_tail(scratch_mapper, search, response, smear, closure, ts)
        if vet:
            self._vetted(vet, 1, ts)
        return resp

    def recognize_all_device(self, range_max, place=None, q_lo=0, n_q=None, stream=None):
        """Every keyframe of a range as a query in one launch (describe_device, then lsd_enqueue_pg_recognize_all_device): per query the
        records and the report recognize_device would leave with that keyframe as the track's last.  n_q None: nodes_cap - q_lo; the
        device clamps to the nodes there are.  find_loops_device chooses among the records.  On `stream`; nothing waits."""
        ts, par = _cuda_stream(stream), pg_place(place)
        lo = int(q_lo)
        nq = self.nodes_cap - lo if n_q is None else int(n_q)
        self.describe_device(range_max, ts)
        self.ctx.enqueue_pg_recognize_all_device(self._head.data_ptr(), self.nodes_cap, self._desc.data_ptr(), par, lo, nq, self._all_recs.data_ptr(),
                                                 self._all_reps.data_ptr(), ts.cuda_stream)
        self._all_q = (lo, nq, int(par.k), int(par.gap), int(par.window))

    def find_loops_device(self, loops=None, stream=None):
        """The distinct loops (lsd_enqueue_pg_loops_device) among the records of the last recognize_all_device, pairs near a closure the
        graph already has left out.  loops: pg_loops().  loop_records() and loops_report() say what was found.  On `stream`; nothing
        waits."""
        if self._all_q is None:
            raise LsdError(LSD_ERR_INVALID, "find_loops_device follows recognize_all_device")
        lo, nq, k = self._all_q[:3]
        par = pg_loops(loops)
        self.ctx.enqueue_pg_loops_device(self._all_recs.data_ptr(), self._all_reps.data_ptr(), lo, nq, k, self._head.data_ptr(), self.nodes_cap,
                                         self._edges.data_ptr(), self.edges_cap, par, self._loops_ws.data_ptr(), self._loops.data_ptr(),
                                         self._loops_rep.data_ptr(), _cuda_stream(stream).cuda_stream)
        self._loops_max = int(par.max_loops)

    def close_all_device(self, scratch_mapper, place=None, loops=None, search=None, response=None, smear=None, closure=None, stream=None,
                         vet=None):
        """Every loop of the graph closed in one pass, on one stream: recognize_all_device over all keyframes, find_loops_device, then for
        m = 0..max_loops-1 lsd_enqueue_pg_loop_select_device and close_device's tail with a near record, a closure report and a response
        record of its own.  An unfilled round ends as NO_ANCHOR.  The anchors' poses do not move between the tails (closures are appended,
        nothing is relaxed); optimize_device and rerender_device follow as after any closure.  range_max is the scratch mapper's.
        Returns the response records, a CUDA uint8 tensor [max_loops, 192]; loop_records(), loops_report() and closure_reports() say
        what came of it.  vet: as close_device's, with one NEW_EDGE query per round (k = 0 .. max_loops - 1; a round that appended
        nothing leaves NO_EDGE).  Nothing waits."""
        import torch
        self._scratch(scratch_mapper)
        ts = _cuda_stream(stream)
        vet = None if vet is None else pg_vet(vet)
        if vet:
            self.snapshot_device(ts)
        self.recognize_all_device(scratch_mapper.range_max, place, 0, None, ts)
        self.find_loops_device(loops, ts)
        gap, window = self._all_q[3:]
        held, resps = [], []
        for m in range(self._loops_max):
            d_near = self._loop_near.data_ptr() + m * PG_NEAR_DTYPE.itemsize
            self.ctx.enqueue_pg_loop_select_device(self._head.data_ptr(), self._nodes.data_ptr(), self.nodes_cap, *self._store_args(), gap, window,
                                                   self._loops.data_ptr(), self._loops_rep.data_ptr(), m, *self._hand_over(d_near), ts.cuda_stream)
            resps.append(self._close_tail(scratch_mapper, search, response, smear, closure, ts, d_near,
                                          self._loop_closure_rep.data_ptr() + m * PG_CLOSURE_REP_DTYPE.itemsize))
            held.append(self._held_close)
        with torch.cuda.stream(ts):
            out = torch.cat(resps, dim=0)
        self._held_close = (held, out)                                       # the launches read them: alive until the next call
        if vet:
            self._vetted(vet, self._loops_max, ts)
        return out

    def relax_device(self, relax=None, stream=None, robust=None, precond=None, **kw):
        """The relaxation (lsd_enqueue_pg_relax_device) of this graph: relax is pg_relax(), or its keywords (iters=, cg_iters=, cg_tol=,
        lambda0=, ..).  The nodes move in place, edge.chi2 and report() are written.  robust: None, or pg_robust() for the robust
        relaxation (lsd_enqueue_pg_relax_robust_device), which also writes robust_report().  precond: None for the two entries above,
        or "block" / "chain" (pg_precond()) for lsd_enqueue_pg_relax_pc_device, which also writes precond_report(): "chain" is the one
        for a long track.  On `stream`; nothing waits."""
        if precond is not None:
            self.ctx.enqueue_pg_relax_pc_device(1, self._head.data_ptr(), self._nodes.data_ptr(), self.nodes_cap, self._edges.data_ptr(),
                                                self.edges_cap, self._ws.data_ptr(), self._relax_rep.data_ptr(), precond, robust,
                                                None if robust is None else self._robust_rep.data_ptr(), self._precond_rep.data_ptr(),
                                                pg_relax(relax, **kw), _cuda_stream(stream).cuda_stream)
            return
        if robust is None:
            self.ctx.enqueue_pg_relax_device(1, self._head.data_ptr(), self._nodes.data_ptr(), self.nodes_cap, self._edges.data_ptr(), self.edges_cap,
                                             self._ws.data_ptr(), self._relax_rep.data_ptr(), pg_relax(relax, **kw), _cuda_stream(stream).cuda_stream)
            return
        self.ctx.enqueue_pg_relax_robust_device(1, self._head.data_ptr(), self._nodes.data_ptr(), self.nodes_cap, self._edges.data_ptr(),
                                                self.edges_cap, self._ws.data_ptr(), self._relax_rep.data_ptr(), pg_robust(robust),
                                                self._robust_rep.data_ptr(), pg_relax(relax, **kw), _cuda_stream(stream).cuda_stream)

    def prune_device(self, gate, max_reject=8, stream=None):
        """The rejection of closures (lsd_enqueue_pg_prune_device): the closure edges that are not disabled and whose chi2 -- the last
        relaxation's -- is not <= gate are candidates; the max_reject (0..64) largest become DISABLED | REJECTED.  prune_report() says
        what was done.  On `stream`; nothing waits."""
        self.ctx.enqueue_pg_prune_device(1, self._head.data_ptr(), self._edges.data_ptr(), self.edges_cap, self._prune_rep.data_ptr(), gate, max_reject,
                                         _cuda_stream(stream).cuda_stream)

    def optimize_device(self, robust, gate, max_reject=8, relax=None, refit=None, stream=None, precond=None):
        """Three launches on one stream: the robust relaxation (robust: pg_robust(); relax: pg_relax()), prune_device(gate, max_reject)
        on the plain chi2 it leaves, and the plain relaxation over the edges that survive (refit: pg_relax(), default: relax).  Huber
        for a first relaxation from drifted poses, Geman-McClure for a closure on a relaxed graph.  report() is the
        refit's, robust_report() and prune_report() those of the first two.  precond: relax_device()'s, for both relaxations
        (precond_report() is the refit's).  Nothing waits."""
        ts = _cuda_stream(stream)
        self.relax_device(relax, ts, robust=robust, precond=precond)
        self.prune_device(gate, max_reject, ts)
        self.relax_device(relax if refit is None else refit, ts, precond=precond)

    def reduce_device(self, reduce=None, stream=None):
        """Redundant keyframes retired and the graph compacted in place (lsd_enqueue_pg_reduce_device), over ALL the
        graph's tracks, its store and its descriptors: a keyframe in a place that `keep` older ones already hold goes where it is an
        inner node of an odometry chain, the chain is contracted across it, and a store that was refusing appends accepts them again.
        reduce: pg_reduce().  The nodes are renumbered: node_map() gives the new index of every old one, and whatever was read back
        EARLIER -- nodes(), edges(), loop_records(), place_records(), marginal_records(), closure reports -- names OLD indices.  The
        graph forgets what it keeps by old index: the last recognize_all_device and find_loops_device (find_loops_device must follow
        a new recognize_all_device), snapshot_device()'s prior (now the reduced graph) and the marginal records.  reduce_report() says
        what was done.  On `stream`; nothing waits."""
        ts = _cuda_stream(stream)
        self.ctx.enqueue_pg_reduce_device(self._head.data_ptr(), self._nodes.data_ptr(), self.nodes_cap, self._edges.data_ptr(), self.edges_cap,
                                          self._tracks.data_ptr(), self.n_tracks, *self._store_args(), self._desc.data_ptr(), reduce,
                                          self._map.data_ptr(), self._reduce_rep.data_ptr(), self._reduce_ws.data_ptr(), ts.cuda_stream)
        self._all_q, self._loops_max = None, 0
        self._marg_q, self._marg_n, self._marg_every = None, 0, False
        self.snapshot_device(ts)

    def reduce_report(self):
        """The last reduce_device's report (PG_REDUCE_REP_DTYPE): a read-back, which waits for the device."""
        return self._read(self._reduce_rep, PG_REDUCE_REP_DTYPE)[0]

    def node_map(self):
        """The last reduce_device's map, int32 [nodes_cap]: the new index of every node there was, -1 for a retired one and behind the
        nodes.  A read-back, which waits for the device."""
        return self._read(self._map, np.dtype("i4"))

    def snapshot_device(self, stream=None):
        """An 8-byte device copy of the head on `stream`: the prior of the NEW_EDGE queries and of the matrix they are solved with --
        the graph as it stands now, in front of the closures that are to be vetted.  Nothing waits."""
        import torch
        with torch.cuda.stream(_cuda_stream(stream)):
            self._prior.copy_(self._head)

    def marginals_device(self, queries=None, marg=None, stream=None, prior=False):
        """Marginal covariances (lsd_enqueue_pg_marginals_device) of this graph at its current poses.  queries: None for every node
        (nodes_cap NODE queries; marginal_records() keeps those of the nodes there are), "tracks" for the last node of every track --
        read from the track records on the device, nothing waits --, "new" for the PG_LOOPS_MAX NEW_EDGE queries k = 0, 1, .., a CUDA
        int32 tensor [n, 4] of (kind, a, b, 0) used where it is, or anything pg_queries() takes, which is uploaded (a host array in
        pageable memory: that copy may wait for the stream).  marg: pg_marg(); its slots are capped by the number of queries, which
        changes no record.  prior: True to solve on the graph as snapshot_device() saw it (what NEW_EDGE queries need).  The records'
        and the workspace's tensors grow with the first call that needs them -- an allocation, never a wait; the tensors they replace
        go back to torch's allocator on `stream`, so ONE stream must carry every marginals_device, vet_device and vetted closure chain of
        a graph (a call on another stream while an earlier one is in flight could be handed memory that is still read).  A graph needs
        a FIXED node: without one the matrix is singular and a solve may still end CONVERGED with an enormous covariance (DESIGN.md
        8.1.20).  On `stream`."""
        import torch
        ts, par = _cuda_stream(stream), pg_marg(marg)
        dev = self._head.device
        with torch.cuda.stream(ts):
            if queries is None:
                q = self._q_every
            elif isinstance(queries, str) and queries == "new":
                q = self._q_new
            elif isinstance(queries, str) and queries == "tracks":
                q = torch.zeros((self.n_tracks, 4), dtype=torch.int32, device=dev)
                q[:, 1] = self._tracks.view(torch.int32)[:, 0]
            elif isinstance(queries, torch.Tensor) and queries.is_cuda:
                if queries.dtype != torch.int32 or queries.dim() != 2 or queries.shape[1] != 4 or not queries.is_contiguous():
                    raise LsdError(LSD_ERR_INVALID, "device queries are a contiguous int32 tensor [n, 4] of (kind, a, b, 0)")
                q = queries
            else:
                if isinstance(queries, torch.Tensor):
                    queries = queries.numpy()
                h = pg_queries(queries)
                q = torch.from_numpy(h.view(np.int32).reshape(len(h), 4).copy()).to(dev)
            n = int(q.shape[0])
            if n > PG_MARG_MAX_QUERIES:
                raise LsdError(LSD_ERR_INVALID, "at most %d queries" % PG_MARG_MAX_QUERIES)
            par = lsd_pg_marg(par.cg_tol, par.cg_iters, par.precond, max(1, min(int(par.slots), n)) if 1 <= par.slots <= PG_MARG_MAX_SLOTS else par.slots, 0)
            need = pg_marginals_workspace_bytes(self.nodes_cap, self.edges_cap, par.precond, par.slots)
            if self._marg_ws is None or self._marg_ws.numel() < need:
                self._marg_ws = torch.zeros(max(need, 8), dtype=torch.uint8, device=dev)
            if self._marg_recs is None or self._marg_recs.shape[0] < n:
                self._marg_recs = torch.zeros((max(n, 1), PG_MARG_REC_DTYPE.itemsize), dtype=torch.uint8, device=dev)
                self._vet_reps = torch.zeros((max(n, 1), PG_VET_REP_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        self.ctx.enqueue_pg_marginals_device(self._head.data_ptr(), self._nodes.data_ptr(), self.nodes_cap, self._edges.data_ptr(), self.edges_cap,
                                             q.data_ptr() if n else None, n, self._marg_ws.data_ptr(), self._marg_recs.data_ptr() if n else None,
                                             self._marg_rep.data_ptr(), par, self._prior.data_ptr() if prior else None, ts.cuda_stream)
        self._marg_q, self._marg_n, self._marg_every = q, n, queries is None

    def vet_device(self, gate, stream=None):
        """The gate (lsd_enqueue_pg_vet_device) on the NEW_EDGE queries of the last marginals_device: a closure whose error at the
        current poses is not plausible under the pair's covariance plus its own becomes DISABLED | REJECTED, as the prune flags an
        edge.  vet_reports() says what was decided.  On a graph without a FIXED node the covariances are enormous where they converge
        at all, and the gate passes everything: it is vacuous there.  On the stream of the marginals_device before it; nothing waits."""
        if self._marg_q is None:
            raise LsdError(LSD_ERR_INVALID, "vet_device follows marginals_device")
        n = self._marg_n
        self.ctx.enqueue_pg_vet_device(self._head.data_ptr(), self._nodes.data_ptr(), self.nodes_cap, self._edges.data_ptr(), self.edges_cap,
                                       self._marg_q.data_ptr() if n else None, self._marg_recs.data_ptr() if n else None, n, gate,
                                       self._vet_reps.data_ptr() if n else None, _cuda_stream(stream).cuda_stream)

    def _vetted(self, vet, n_new, ts):
        """Behind the closures of a chain that began with snapshot_device(): the marginals of the first n_new new edges, then the gate."""
        self.marginals_device(self._q_new[:n_new], vet["marg"], ts, prior=True)
        self.vet_device(vet["gate"], ts)

    def marginal_records(self):
        """The last marginals_device's records (PG_MARG_REC_DTYPE, one per query; for queries=None those of the nodes there are): a
        read-back, which waits for the device."""
        if self._marg_q is None:
            return np.zeros(0, PG_MARG_REC_DTYPE)
        n = self.head()[0] if self._marg_every else self._marg_n
        return self._read(self._marg_recs, PG_MARG_REC_DTYPE)[:n]

    def marginals_report(self):
        """The last marginals_device's report (PG_MARG_REP_DTYPE): a read-back, which waits for the device."""
        return self._read(self._marg_rep, PG_MARG_REP_DTYPE)[0]

    def vet_reports(self):
        """The last vet_device's reports (PG_VET_REP_DTYPE, one per query of the marginals before it): a read-back."""
        if self._vet_reps is None:
            return np.zeros(0, PG_VET_REP_DTYPE)
        return self._read(self._vet_reps, PG_VET_REP_DTYPE)[:self._marg_n]

    def fix(self, node, stream=None):
        """Sets LSD_PG_NODE_FIXED on a node, on `stream`; nothing waits."""
        import torch
        n = int(node)
        if not 0 <= n < self.nodes_cap:
            raise LsdError(LSD_ERR_INVALID, "node must be 0..nodes_cap-1")
        with torch.cuda.stream(_cuda_stream(stream)):
            self._nodes.view(torch.int32)[n, 12] |= PG_NODE_FIXED            # (flags: byte 48 of the record)

    def _read(self, t, dtype):
        return t.cpu().numpy().reshape(-1).view(dtype).copy()

    def head(self):
        """(n_nodes, n_edges), clamped to the capacities: a read-back, which waits for the device."""
        h = self._read(self._head, PG_HEAD_DTYPE)[0]
        return min(max(int(h["n_nodes"]), 0), self.nodes_cap), min(max(int(h["n_edges"]), 0), self.edges_cap)

    def nodes(self):
        """The nodes as a numpy array of PG_NODE_DTYPE [n_nodes]: a read-back, which waits for the device."""
        return self._read(self._nodes, PG_NODE_DTYPE)[:self.head()[0]]

    def edges(self):
        """The edges as a numpy array of PG_EDGE_DTYPE [n_edges]: a read-back, which waits for the device."""
        return self._read(self._edges, PG_EDGE_DTYPE)[:self.head()[1]]

    def report(self):
        """The last relax_device's report (PG_RELAX_REP_DTYPE): a read-back, which waits for the device."""
        return self._read(self._relax_rep, PG_RELAX_REP_DTYPE)[0]

    def robust_report(self):
        """The second report (PG_ROBUST_REP_DTYPE) of the last ROBUST relaxation -- relax_device(robust=) or optimize_device; a plain
        relax_device after it leaves this record as it was, so it is older than report() then.  A read-back, which waits for the device."""
        return self._read(self._robust_rep, PG_ROBUST_REP_DTYPE)[0]

    def precond_report(self):
        """The preconditioner's report (PG_PRECOND_REP_DTYPE) of the last relaxation that was given precond=: the chain edges, the paths,
        the longest path's nodes, the outer iterations that fell back to the diagonal blocks.  A read-back, which waits for the device."""
        return self._read(self._precond_rep, PG_PRECOND_REP_DTYPE)[0]

    def prune_report(self):
        """The last prune_device's report (PG_PRUNE_REP_DTYPE): a read-back, which waits for the device."""
        return self._read(self._prune_rep, PG_PRUNE_REP_DTYPE)[0]

    def closure_report(self):
        """(the near record PG_NEAR_DTYPE, the closure report PG_CLOSURE_REP_DTYPE) of the last close_device: a read-back."""
        return self._read(self._near, PG_NEAR_DTYPE)[0], self._read(self._closure_rep, PG_CLOSURE_REP_DTYPE)[0]

    def place_report(self):
        """The last recognize_device's report (PG_PLACE_REP_DTYPE): a read-back, which waits for the device."""
        return self._read(self._place_rep, PG_PLACE_REP_DTYPE)[0]

    def place_records(self):
        """The last recognize_device's places (PG_PLACE_REC_DTYPE [k], anchor -1 in a round that found none): a read-back."""
        return self._read(self._place_recs, PG_PLACE_REC_DTYPE)[:getattr(self, "_place_k", PG_PLACE_MAX)]

    def loop_records(self):
        """The last find_loops_device's loops (PG_LOOP_REC_DTYPE [max_loops], query -1 in a round that found none): a read-back."""
        return self._read(self._loops, PG_LOOP_REC_DTYPE)[:self._loops_max]

    def loops_report(self):
        """The last find_loops_device's report (PG_LOOPS_REP_DTYPE): a read-back, which waits for the device."""
        return self._read(self._loops_rep, PG_LOOPS_REP_DTYPE)[0]

    def closure_reports(self):
        """(the near records PG_NEAR_DTYPE [max_loops], the closure reports PG_CLOSURE_REP_DTYPE [max_loops]) of the last
        close_all_device, one per round: a read-back."""
        n = self._loops_max
        return self._read(self._loop_near, PG_NEAR_DTYPE)[:n], self._read(self._loop_closure_rep, PG_CLOSURE_REP_DTYPE)[:n]

    def append_report(self):
        """The last append's report (PG_APPEND_REP_DTYPE): a read-back, which waits for the device."""
        return self._read(self._append_rep, PG_APPEND_REP_DTYPE)[0]

    def disable_edges(self, chi2_above):
        """Sets LSD_PG_EDGE_DISABLED on every edge whose chi2 (the last relaxation's) exceeds chi2_above; returns their indices.  A host
        convenience over edges(): it waits for the device."""
        import torch
        ed = self.edges()
        hit = np.flatnonzero(ed["chi2"] > float(chi2_above))
        if len(hit):
            ed["flags"][hit] |= PG_EDGE_DISABLED
            self._edges[:len(ed)].copy_(torch.from_numpy(ed.view(np.uint8).reshape(len(ed), -1)))
        return hit


class _MapSlot:
    """One of a Localizer's two maps on the device: the map bytes, the cache, the line records and their count, the geometry the ticks
    pass with them, and the two events of the hand-over."""

    def __init__(self):
        self.cells = self.cap_lines = 0          # what the tensors hold (grow-only)
        self.map = self.mc = self.lines = self.count = None
        self.cols = self.rows = 0
        self.lines_cap = 0                       # the records the map's update could write: what the ticks hold the count to
        self.n_host = None                       # set_map: the count as the host knows it; None: only the device does (set_map_device)
        self.map_param = None
        self.grid = None                         # the update's input, alive until the slot is filled again
        self.ready = None                        # recorded behind the update that filled the slot
        self.waited = set()                      # streams that have been put behind `ready`
        self.last_stream = None                  # the stream of the last tick that read the slot (None: no tick since it was filled)
        self.idle = None                         # recorded behind that tick when the ticks moved on to the other slot


class _MapPair:
    """The two slots of one map and the hand-over between them, as Localizer and -- per map id -- FleetLocalizer use it: the ticks read
    slot `cur`; a new map is made in the other one, on any stream, behind the events of that slot's last readers and last update, and
    handed over through `ready`; nothing waits on the host unless a slot has to grow."""

    def __init__(self):
        self.slots, self.cur = (_MapSlot(), _MapSlot()), 1

    @property
    def current(self):
        return self.slots[self.cur]

    @staticmethod
    def fit(slot, cells, n_lines, keep=False):
        """The slot's tensors for at least `cells` cells and n_lines records.  Growing them waits -- on the host -- for the ticks that
        still read the slot and for the update that filled it; keep: what it holds moves over."""
        import torch
        if slot.cells >= cells and slot.cap_lines >= n_lines:
            return
        for ev in (slot.idle, slot.ready):
            if ev is not None:
                ev.synchronize()
        if slot.last_stream is not None:
            slot.last_stream.synchronize()
        cells, n_lines = max(cells, slot.cells), max(n_lines, slot.cap_lines)
        z = lambda count, dt: torch.zeros(count, dtype=dt, device="cuda")
        new = (z(cells, torch.uint8), z(cells, torch.float64), z(n_lines * 80, torch.uint8), z(1, torch.int32))
        if keep and slot.cells:
            for dst, src in zip(new, (slot.map, slot.mc, slot.lines, slot.count)):
                dst[:src.numel()].copy_(src)
        # the blocks may have served other work of this stream, and an update may write them from another one: that work is over first
        torch.cuda.current_stream().synchronize()
        slot.map, slot.mc, slot.lines, slot.count = new
        slot.cells, slot.cap_lines = cells, n_lines

    def target(self, stream, cells, n_lines):
        """The slot the ticks are not reading, large enough, with `stream` behind its last readers and its last update."""
        slot = self.slots[1 - self.cur]
        self.fit(slot, cells, n_lines)
        for ev in (slot.idle, slot.ready):
            if ev is not None:
                stream.wait_event(ev)
        return slot

    def hand_over(self, slot, stream, cols, rows, lines_cap, n_host, map_param, grid=None):
        """`slot` has been filled on `stream`: the ticks from now on read it, once their stream is behind the update."""
        import torch
        slot.ready = torch.cuda.Event()
        slot.ready.record(stream)
        slot.waited = {stream.cuda_stream}
        slot.cols, slot.rows, slot.lines_cap, slot.n_host, slot.map_param, slot.grid = cols, rows, lines_cap, n_host, map_param, grid
        slot.idle = None
        old = self.slots[self.cur]
        if old is not slot and old.last_stream is not None:          # behind the last tick that read the map the ticks now leave
            old.idle = torch.cuda.Event()
            old.idle.record(old.last_stream)
            old.last_stream = None
        self.cur = self.slots.index(slot)

    def read_by(self, ts):
        """The slot a tick on torch stream `ts` reads: the first tick of a stream on a new map goes behind its update."""
        m = self.slots[self.cur]
        if ts.cuda_stream not in m.waited:
            ts.wait_event(m.ready)
            m.waited.add(ts.cuda_stream)
        m.last_stream = ts
        return m


def _frame_of(map_param):
    """(mapResol, mapOriX, mapOriY) of a map_param: the frame carries made on that map are in."""
    return tuple(float(v) for v in map_param[2:5])


def _compose_rebase(pending, frame_from, frame_to):
    """A re-base still pending followed by another: the earliest `from`, the latest `to` (None: they cancel)."""
    f = pending[0] if pending else frame_from
    return None if f == frame_to else (f, frame_to)


def _check_n_beams(n_beams):
    """n_beams of Localizer / FleetLocalizer: readings per scan, 1 .. LSD_SCAN_MAX_LEN."""
    n = int(n_beams)
    if n < 1:
        raise LsdError(LSD_ERR_INVALID, "n_beams must be at least 1")
    if n > LSD_SCAN_MAX_LEN:
        raise LsdError(LSD_ERR_UNSUPPORTED, "n_beams above LSD_SCAN_MAX_LEN = %d" % LSD_SCAN_MAX_LEN)
    return n


class _Ticks:
    """Localizer and FleetLocalizer but for their argument adapters: the robots' carries on the device, the map side -- one _MapPair per
    map (one for Localizer), the hand-over, the pending re-bases, the one map-side context --, the FeatureScan staging, and the tick
    (step, step_device).  n_beams: the readings per scan the ticks take (the staging, the ingest and FeatureScan strides; 360, the
    reference's lidar, unless the constructor says otherwise; above 1024 the context's scan capacity is raised to it).  A subclass supplies three hooks of the map side (_rebase_key, _map_changed, _carve), the tick's two launches
    against its map or maps (_feature_scan, _loop) and the texts of step()'s two map errors."""

    _GAVE_UP = "the detector gave the map up (count -1): the tick saw no map lines"
    _OVER = "the map has %(n)d lines, its slot holds %(cap)d (reserve_map): the tick used the first %(cap)d"

    def __init__(self, ctx, n_robots, pts_cap, n_maps=1, n_beams=360):
        import torch
        self.ctx = ctx or default_context()
        self.n_robots, self.pts_cap = int(n_robots), int(pts_cap)
        self.n_beams = _check_n_beams(n_beams)
        self._IN_B = self._in_b(self.n_beams)
        if self.n_beams > max(1024, self.ctx.scan_capacity):                 # a long lidar: the context takes its scans from now on
            self.ctx.set_scan_capacity(self.n_beams)
        self._carry = torch.zeros(self.n_robots * FA_CARRY_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        self._pairs = [_MapPair() for _ in range(n_maps)]                    # per map: the slot the ticks read, and the other one
        self._caps = [512] * n_maps                                          # per map: the line records a device-made map keeps (reserve_map)
        self._rebases = {}                                                   # map -> (from, to): due at the next tick
        self._map_ctx, self._map_geom = None, (0, 0)                         # the map side's context, the largest geometry reserved for it
        self._cap = 0
        self._held = None
        self._last_tick = None                                               # (S, k, stream, robots) of the last tick enqueued
        self._tail_b = 4 * len(self._pairs)                                  # bytes behind the outputs: the map line counts of step()
        # every hand-over re-bases, as set_map*(..., rebase=True) does for one: the setting of a site whose maps grow.  It is also how
        # Localizer.set_map_device, whose parameter list is fixed, is told to re-base.
        self.rebase_on_hand_over = False

    # ---- the three hooks of the map side ----
    def _rebase_key(self, i):
        """(d_key, key) of lsd_enqueue_fa_carry_rebase_device: the robots whose carries a pending re-base of map i moves."""
        raise NotImplementedError

    def _map_changed(self, i):
        """Map i has been handed over, or its current slot's tensors have moved: whatever else names them follows."""

    def _carve(self, i):
        """A tick of no frames on the current torch stream: nothing is launched, the workspace of n_robots sequences against the line
        capacity reserve_map has just set for map i is carved."""
        raise NotImplementedError

    # ---- the map side, per map index ----
    def _map_context(self):
        # The map side has a context of its own, one for every map: the detector's workspace and createMapCache's
        # scratch belong to a context, which serves one stream at a time, and the ticks' context is busy on theirs while an update runs
        # on a side stream.
        if self._map_ctx is None:
            self._map_ctx = Context(self.ctx.device)
        return self._map_ctx

    def _flush_rebase(self):
        """Enqueues, on the current torch stream, every re-base that a set_map*(..., rebase=True) left pending for the next tick."""
        if self._rebases:
            import torch
            stream = torch.cuda.current_stream().cuda_stream
            pending, self._rebases = self._rebases, {}
            for i, (f, t) in pending.items():                                # (a key is read when the kernel runs)
                self.ctx.enqueue_fa_carry_rebase_device(self._carry.data_ptr(), self.n_robots, *self._rebase_key(i), f, t, stream)

    def _hand_over(self, i, slot, stream, cols, rows, lines_cap, n_host, map_param, grid, rebase):
        """Map i's hand-over: the pair's, what _map_changed adds, and -- rebase -- the carries' move to the new map's frame left pending
        for the next tick."""
        pair = self._pairs[i]
        if (rebase or self.rebase_on_hand_over) and pair.current.map_param is not None:
            r = _compose_rebase(self._rebases.get(i), _frame_of(pair.current.map_param), _frame_of(map_param))
            self._rebases.pop(i, None)
            if r is not None:
                self._rebases[i] = r
        pair.hand_over(slot, stream, cols, rows, lines_cap, n_host, map_param, grid)
        self._map_changed(i)

    def _set_map(self, i, map_cache, map_lines, map_param, rebase):
        import torch
        mc = map_cache if isinstance(map_cache, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(map_cache, np.float64))
        ml = np.ascontiguousarray(map_lines, LINE_DTYPE).reshape(-1)
        mp = tuple(float(v) for v in map_param)
        if mc.dim() != 2 or not mc.numel() or len(mp) != 5 or not mp[2] > 0:
            raise LsdError(LSD_ERR_INVALID, "map_cache is [rows, cols], map_param (oriMapCol, oriMapRow, mapResol > 0, mapOriX, mapOriY)")
        if len(ml) * 360 > 1 << 26:
            raise LsdError(LSD_ERR_UNSUPPORTED, "map lines x 360 pairs per robot exceed 1 << 26")
        if rebase or self.rebase_on_hand_over:
            map_frame(mp)                                                    # a frame the re-base would refuse: before anything is enqueued
        rows, cols = mc.shape
        stream = torch.cuda.current_stream()
        slot = self._pairs[i].target(stream, rows * cols, max(len(ml), 1))
        slot.mc[:rows * cols].copy_(mc.reshape(-1))
        if len(ml):
            slot.lines[:80 * len(ml)].copy_(torch.from_numpy(ml.view(np.uint8).reshape(-1).copy()))
        slot.count.fill_(len(ml))
        self._hand_over(i, slot, stream, cols, rows, max(len(ml), 1), len(ml), mp, None, rebase)

    def _reserve_map(self, i, cols, rows, lines_cap):
        import torch
        cols, rows, lines_cap = int(cols), int(rows), int(lines_cap)
        if cols <= 0 or rows <= 0 or lines_cap <= 0:
            raise LsdError(LSD_ERR_INVALID, "cols, rows and lines_cap must be positive")
        if lines_cap * 360 > 1 << 26:
            raise LsdError(LSD_ERR_UNSUPPORTED, "lines_cap x 360 pairs per robot exceed 1 << 26")
        torch.cuda.synchronize()
        pair = self._pairs[i]
        for j, slot in enumerate(pair.slots):
            pair.fit(slot, rows * cols, lines_cap, keep=j == pair.cur)
        self._map_changed(i)                                                 # (the current slot's tensors may have moved)
        self._caps[i] = lines_cap
        self._map_geom = (max(self._map_geom[0], cols), max(self._map_geom[1], rows))
        self._map_context().reserve_map_update(*self._map_geom)
        self._staging(self.n_robots)
        self._carve(i)
        torch.cuda.synchronize()

    def _set_map_device(self, i, d_grid, oriMapCol, oriMapRow, mapResol, mapOriX, mapOriY, stream, rebase):
        cols, rows = int(oriMapCol), int(oriMapRow)
        grid = _occupancy_grid(d_grid, cols, rows, self.ctx.device)
        stream = _cuda_stream(stream)
        mp = (float(cols), float(rows), float(mapResol), float(mapOriX), float(mapOriY))
        if not mp[2] > 0:
            raise LsdError(LSD_ERR_INVALID, "mapResol must be > 0")
        if rebase or self.rebase_on_hand_over:
            map_frame(mp)                                                    # a frame the re-base would refuse: before anything is enqueued
        mctx, cap = self._map_context(), self._caps[i]
        slot = self._pairs[i].target(stream, rows * cols, cap)
        mctx.enqueue_map_update_device(grid.data_ptr(), cols, rows, mp[2], 2.0, slot.map.data_ptr(), slot.mc.data_ptr(), slot.lines.data_ptr(), cap,
                                       slot.count.data_ptr(), None, None, stream.cuda_stream)
        self._hand_over(i, slot, stream, cols, rows, cap, None, mp, grid, rebase)

    def reset(self, robots, odom0=(0.0, 0.0, 0.0), state=None):
        """Restarts the given robots at the driver's first frame: lsd_fa_carry_init(state, odom0) (odom0 [3], or one row per robot).  A
        re-base that is pending (set_map*(..., rebase=True) without a tick since) is enqueued first, on the current stream: a `state`
        given here is in the frame of the map the next tick reads."""
        import torch
        idx = [int(r) for r in robots]
        if not idx:
            return
        self._flush_rebase()
        o = np.broadcast_to(np.asarray(odom0, np.float64).reshape(-1, 3), (len(idx), 3))
        rec = np.stack([Context.fa_carry_init(state, o[i]) for i in range(len(idx))])
        self._carry.view(self.n_robots, -1)[torch.tensor(idx, device="cuda")] = torch.from_numpy(rec.view(np.uint8).reshape(len(idx), -1)).cuda()

    @property
    def carries(self):
        """The robots' carries, FA_CARRY_DTYPE [n_robots] on the host (a checkpoint), in the frame of the map the next tick reads (a
        pending re-base is enqueued first)."""
        self._flush_rebase()
        return self._carry.cpu().numpy().view(FA_CARRY_DTYPE).copy()

    @carries.setter
    def carries(self, rec):
        import torch
        rec = np.ascontiguousarray(rec, FA_CARRY_DTYPE).reshape(-1)
        if len(rec) != self.n_robots:
            raise LsdError(LSD_ERR_INVALID, "one carry per robot")
        self._flush_rebase()
        self._carry.copy_(torch.from_numpy(rec.view(np.uint8).copy()))

    # per frame slot: the tick's inputs (one upload) the RAW scan (n_beams x 2 doubles, or less: the LaserScan floats), the odometry row,
    # the take flag; the scan as FeatureScan reads it (k_ingest's output) and its length; its outputs (one read-back) the state, the
    # report, FeatureScan's line and pixel counts.  _IN_B is per instance (__init__); the class's is the reference lidar's, 360 readings.
    @staticmethod
    def _in_b(n_beams):
        return 16 * n_beams + 24 + 4

    _IN_B, _OUT_B = 16 * 360 + 24 + 4, FA_STATE_DTYPE.itemsize + FA_REPORT_DTYPE.itemsize + 8

    def _staging(self, n):
        import torch
        if n <= self._cap:
            return
        z = lambda count, dt: torch.zeros(count, dtype=dt, device="cuda")
        self._in, self._out = z(n * self._IN_B, torch.uint8), z(n * self._OUT_B + self._tail_b, torch.uint8)     # (+ the map line counts of step())
        self._scans, self._lens = z(n * self.n_beams * 2, torch.float64), z(n, torch.int32)
        self._lines, self._pts = z(n * 360 * 80, torch.uint8), z(n * self.pts_cap * 3, torch.float64)
        self._lp, self._sz = z(n * 2, torch.float64), z(n * 2, torch.int32)
        self._cap = n

    def _n_frames(self, n_frames, S, k):
        nf = np.full(S, k, np.int32) if n_frames is None else np.ascontiguousarray(n_frames, np.int32).reshape(S)
        if (nf < 0).any() or (nf > k).any():
            raise LsdError(LSD_ERR_INVALID, "n_frames outside 0..k")
        return nf

    def _feature_scan(self, n, k, d_scans, d_lens, d_n_lines, d_n_pts, stream):
        """FeatureScan of the tick's n = S * k scans into the staging (self._lines, self._pts, self._lp, self._sz) and the two count rows."""
        raise NotImplementedError

    def _loop(self, S, k, nf, d_n_lines, d_n_pts, d_od, d_states, d_reports, stream):
        """The resume loop on what _feature_scan left, against the current slot of the map or of every map."""
        raise NotImplementedError

    def _enqueue(self, S, k, nf, d_raw, d_ranges, d_ami, n_beams, d_take, d_od):
        """The tick on the current torch stream, every input on the device: ingest, FeatureScan, then -- behind the update of every map
        whose current slot this stream has not read yet, and behind the pending re-bases -- the resume loop.  Returns the byte sizes of
        the states and the reports in self._out."""
        import torch
        n = S * k
        b_st, b_rp = n * FA_STATE_DTYPE.itemsize, n * FA_REPORT_DTYPE.itemsize
        self._out[:b_st + b_rp].zero_()
        d_sc, d_ln, d_out = self._scans.data_ptr(), self._lens.data_ptr(), self._out.data_ptr()
        d_st, d_rp, d_nl = d_out, d_out + b_st, d_out + b_st + b_rp
        d_np = d_nl + 4 * n
        cx, ts = self.ctx, torch.cuda.current_stream()
        stream = ts.cuda_stream
        if d_raw is not None:
            cx.enqueue_scan_ingest_device(d_raw, n, self.n_beams, d_take, d_sc, d_ln, self.n_beams, stream)
        else:
            cx.enqueue_laserscan_ingest_device(d_ranges, d_ami, n, n_beams, d_take, d_sc, d_ln, self.n_beams, stream)
        self._feature_scan(n, k, d_sc, d_ln, d_nl, d_np, stream)
        for pair in self._pairs:
            pair.read_by(ts)                                                 # the first tick of this stream on a new map: behind its update
        self._flush_rebase()                                                 # and, in front of the loop, the carries into that map's frame
        self._loop(S, k, nf, d_nl, d_np, d_od, d_st, d_rp, stream)
        self._last_tick = (S, k, ts, self._tick_robots())                    # what integrate_last_tick reads
        return b_st, b_rp

    def _tick_robots(self):
        """The host's record of which robots the tick being enqueued belongs to, for integrate_last_tick (Localizer: all of them)."""
        return None

    def _integrate_last_tick(self, mapper, robots):
        """integrate_last_tick for the robots `robots` (ascending indices): one launch per run of neighbouring robots, on the tick's
        stream, reading the tick's staging -- slot s * k + t holds frame t of robot s: its packed scan and length (k_ingest's output)
        and, in the read-back block, the state the frame produced, whose first three doubles are the pose (pitch 720)."""
        if self._last_tick is None:
            raise LsdError(LSD_ERR_INVALID, "no tick has been enqueued yet")
        if not isinstance(mapper, GridMapper):
            raise LsdError(LSD_ERR_INVALID, "mapper must be a GridMapper")
        S, k, ts, _ = self._last_tick
        d_sc, d_ln, d_st = self._scans.data_ptr(), self._lens.data_ptr(), self._out.data_ptr()
        b_state, b_scan = FA_STATE_DTYPE.itemsize, 16 * self.n_beams
        for first, count in self._runs(robots, k):
            mapper._enqueue(self.ctx, d_sc + first * b_scan, d_ln + first * 4, count, self.n_beams, d_st + first * b_state, b_state,
                            ts.cuda_stream)

    def _append_last_tick(self, graph, robot, track, append):
        """append_last_tick for one robot: its k slots of the tick's staging (scans, lengths, the states at pitch 720) as the candidates of
        PoseGraph's append, on the tick's stream."""
        if self._last_tick is None:
            raise LsdError(LSD_ERR_INVALID, "no tick has been enqueued yet")
        if not isinstance(graph, PoseGraph) or not 0 <= int(robot) < self.n_robots:
            raise LsdError(LSD_ERR_INVALID, "graph must be a PoseGraph, robot one of the localizer's")
        S, k, ts, _ = self._last_tick
        first, b_state = int(robot) * k, FA_STATE_DTYPE.itemsize
        graph._append(self._scans.data_ptr() + first * 16 * self.n_beams, self._lens.data_ptr() + first * 4, k, self.n_beams,
                      self._out.data_ptr() + first * b_state, b_state, track, append, ts)

    @staticmethod
    def _runs(robots, k):
        """(first slot, slot count) of every run of neighbouring robots among `robots` (ascending indices), k slots per robot."""
        robots = [int(r) for r in robots]
        a = 0
        while a < len(robots):
            b = a
            while b + 1 < len(robots) and robots[b + 1] == robots[b] + 1:
                b += 1
            yield robots[a] * k, (robots[b] - robots[a] + 1) * k
            a = b + 1

    def _refine_and_integrate_last_tick(self, mapper, robots, key, search, refresh, smear, block, response, integrate_at, correct):
        """refine_and_integrate_last_tick for the robots `robots` (ascending indices; None: all of them, in one chain): GridMapper._chain per
        run of neighbouring robots on the tick's staging, the lookup plane refreshed once in front of the first; then, with `correct`, the
        correction of the carries behind the response stage, for the sequences `key` = (d_key, key) selects on the device."""
        import torch
        if self._last_tick is None:
            raise LsdError(LSD_ERR_INVALID, "no tick has been enqueued yet")
        if not isinstance(mapper, GridMapper):
            raise LsdError(LSD_ERR_INVALID, "mapper must be a GridMapper")
        if correct is not None and response is None:
            raise LsdError(LSD_ERR_INVALID, "correct needs the response stage: give response")
        par = None if correct is None else fa_correct(correct)
        S, k, ts, _ = self._last_tick
        d_sc, d_ln, d_st = self._scans.data_ptr(), self._lens.data_ptr(), self._out.data_ptr()
        b_state, b_scan = FA_STATE_DTYPE.itemsize, 16 * self.n_beams
        chain = lambda first, count, fresh: mapper._chain(self.ctx, d_sc + first * b_scan, d_ln + first * 4, count, self.n_beams,
                                                          d_st + first * b_state, b_state, search, ts, block, response=response, integrate=True,
                                                          refresh=fresh, smear=smear, integrate_at=integrate_at)
        if robots is None:
            got = chain(0, S * k, refresh)
            parts = list(got) if isinstance(got, tuple) else [got]
        else:
            if integrate_at not in ("match", "response") or (integrate_at == "response" and response is None):
                raise LsdError(LSD_ERR_INVALID, "integrate_at is 'match' or, with response given, 'response'")
            widths = [GRID_MATCH_DTYPE.itemsize] + ([GRID_RESPONSE_DTYPE.itemsize] if response is not None else [])
            with torch.cuda.stream(ts):
                parts = [torch.zeros((S * k, w), dtype=torch.uint8, device=mapper._planes.device) for w in widths]
            if refresh:
                mapper.likelihood_device(smear, ts, block)                   # once: every run is matched on the plane of before the call
            held = []
            for first, count in self._runs(robots, k):
                got = chain(first, count, False)
                got = got if isinstance(got, tuple) else (got,)
                with torch.cuda.stream(ts):
                    for whole, run in zip(parts, got):
                        whole[first:first + count].copy_(run)
                held.append(got)
            mapper._held_rec = held                                          # the integrations read them: alive until the next ones
        if par is not None:
            parts.append(self._correct_last_tick(parts[-1], par, key))
        return tuple(parts) if len(parts) > 1 else parts[0]

    def _correct_last_tick(self, responses, correct, key):
        """correct_last_tick for the sequences `key` = (d_key, key) selects on the device: one launch on the tick's stream, the poses the
        tick's states (pitch 720), the carries the localiser's own.  The reports: a new CUDA uint8 tensor [n_robots, 48], zero bytes for a
        robot the key leaves out."""
        import torch
        if self._last_tick is None:
            raise LsdError(LSD_ERR_INVALID, "no tick has been enqueued yet")
        S, k, ts, _ = self._last_tick
        if (not isinstance(responses, torch.Tensor) or not responses.is_cuda or not responses.is_contiguous() or
                responses.numel() * responses.element_size() != S * k * GRID_RESPONSE_DTYPE.itemsize):
            raise LsdError(LSD_ERR_INVALID, "responses must be a contiguous CUDA tensor of n_robots * k records of 192 bytes")
        par = fa_correct(correct)
        with torch.cuda.stream(ts):
            rep = torch.zeros((S, FA_CORRECT_DTYPE.itemsize), dtype=torch.uint8, device=responses.device)
        self.ctx.enqueue_fa_carry_correct_device(self._carry.data_ptr(), S, k, self._out.data_ptr(), FA_STATE_DTYPE.itemsize, responses.data_ptr(),
                                                 key[0], key[1], par, rep.data_ptr(), ts.cuda_stream)
        self._held_correct = responses                                       # the launch reads it: alive until the next one
        return rep

    def _checked_tick(self, mapper):
        if self._last_tick is None:
            raise LsdError(LSD_ERR_INVALID, "no tick has been enqueued yet")
        if not isinstance(mapper, GridMapper):
            raise LsdError(LSD_ERR_INVALID, "mapper must be a GridMapper")
        return self._last_tick

    def _relocate_last_tick(self, mapper, key, locate, seed, max_lost, refresh, smear, response, search, stats, write=True, tight=None):
        """relocate_last_tick for the sequences `key` = (d_key, key) selects on the device, on the tick's stream and behind the tick: the
        gather (the carries, the tick's states at pitch 720, its ingested scans), the mapper's locate on the gathered batch, with `response`
        a match of zero window at the locate records (pitch 64: the response stage reads a match record's di / dj / da, which a locate
        record does not have) and the response stage at those, then the seed (write=False: none, and no report)."""
        import torch
        S, k, ts, _ = self._checked_tick(mapper)
        n, par = int(max_lost), fa_seed(seed) if write else None
        if not 1 <= n <= 4096:
            raise LsdError(LSD_ERR_INVALID, "max_lost must be 1..4096")
        rp = None if response is None else grid_response(response)
        if rp is not None:
            se = grid_search(search)
            se = lsd_grid_search(0, 0, 0, se.ang_step, se.min_beams, se.min_num, se.min_den)
        locate = grid_locate(locate, cols=mapper.cols, rows=mapper.rows)         # (refused here: before the gather is enqueued)
        tight = grid_locate_tight(tight)
        dev, B = self._carry.device, self.n_beams
        with torch.cuda.stream(ts):
            sc = torch.zeros((n, B, 2), dtype=torch.float64, device=dev)         # rows past the gathered ones keep these zeros
            ln, pick, n_lost = (torch.empty(c, dtype=torch.int32, device=dev) for c in (n, n, 2))
            rep = torch.empty((n, FA_SEED_DTYPE.itemsize), dtype=torch.uint8, device=dev) if write else None
        cx, d_cy = self.ctx, self._carry.data_ptr()
        cx.enqueue_fa_lost_gather_device(d_cy, S, k, self._out.data_ptr(), FA_STATE_DTYPE.itemsize, self._scans.data_ptr(), self._lens.data_ptr(), B,
                                         key[0], key[1], n, sc.data_ptr(), ln.data_ptr(), pick.data_ptr(), n_lost.data_ptr(), ts.cuda_stream)
        got = mapper._enqueue_locate(cx, sc.data_ptr(), ln.data_ptr(), n, B, locate, refresh, smear, stats, ts, tight)
        parts = list(got) if stats else [got]
        resp = rec0 = None
        if rp is not None:
            rec0 = mapper._enqueue_match(cx, sc.data_ptr(), ln.data_ptr(), n, B, parts[0].data_ptr(), GRID_LOCATE_DTYPE.itemsize, se, ts)
            resp = mapper._enqueue_response(cx, sc.data_ptr(), ln.data_ptr(), n, B, parts[0].data_ptr(), GRID_LOCATE_DTYPE.itemsize, rec0.data_ptr(),
                                            se, rp, ts)
            parts.append(resp)
        if write:
            cx.enqueue_fa_carry_seed_device(d_cy, S, k, pick.data_ptr(), n, parts[0].data_ptr(), None if resp is None else resp.data_ptr(), par,
                                            rep.data_ptr(), ts.cuda_stream)
        self._held_relocate = (sc, ln, rec0, pick, n_lost, rep) + tuple(parts)  # the launches read them: alive until the next call
        return (pick, n_lost) + tuple(parts) + ((rep,) if write else ())

    def step(self, lidar=None, odom=None, n_frames=None, *, ranges=None, angle_min_inc=None):
        """lidar float64 [S, k, n_beams, 2] raw frames (range, angle) as laserCallback reads them (infinite ranges dropped as lidar_frames
        does, on the device: k_ingest), odom float64 [S, k, 3] the NEW odometry row of each frame (Odom[cnt_frame]); S = n_robots; n_beams
        is the constructor's (default 360, the reference's lidar).  Instead of lidar: ranges float32 [S, k, B <= n_beams] and
        angle_min_inc float32 [S, k, 2], the fields of sensor_msgs/LaserScan messages (see step_device).  A robot whose lidar has fewer
        readings than n_beams pads each scan at the tail with +inf ranges, which the ingest drops: its scan is then exactly the shorter
        one (in the LaserScan layout the kept beams' angles, angle_min + i * angle_increment, do not depend on B).  n_frames: frames per robot this tick (default k each; a robot with 0 is left untouched).  Returns (states
        FA_STATE_DTYPE [S, k], reports FA_REPORT_DTYPE [S, k]); slots past a robot's n_frames are zero, and so are those of a robot that
        sits out (FleetLocalizer).  Raises LsdError(LSD_ERR_CAPACITY) with (states, reports) in `partial` if a scan marks more than
        pts_cap pixels or has more than 360 lines (the records are then computed from the stored part), as lsd_localize does.  One upload
        (the raw frames, the odometry, the take flags), the device tick of step_device, one read-back.  Raises
        LsdError(LSD_ERR_CAPACITY) as well, with (states, reports) in `partial`, when a map the tick used was made on the device
        (set_map_device) and has more lines than its slots hold (the records of its robots are computed from the first lines_cap of
        them), and LsdError(LSD_ERR_INTERNAL) when such a map's count is -1 (its robots saw no map lines); FleetLocalizer's message
        names the map id, and the robots on other maps are not affected."""
        import torch
        if (lidar is None) == (ranges is None):
            raise LsdError(LSD_ERR_INVALID, "give either lidar or ranges")
        if ranges is None:
            src = np.asarray(lidar, np.float64)
            S, k = src.shape[0], src.shape[1]
            if S != self.n_robots or src.shape[2:] != (self.n_beams, 2) or k < 1:
                raise LsdError(LSD_ERR_INVALID, "lidar must be [n_robots, k >= 1, %d, 2]" % self.n_beams)
            n_beams = self.n_beams
        else:
            src = np.asarray(ranges, np.float32)
            if src.ndim != 3 or src.shape[0] != self.n_robots or src.shape[1] < 1 or not 1 <= src.shape[2] <= self.n_beams:
                raise LsdError(LSD_ERR_INVALID, "ranges must be [n_robots, k >= 1, 1 <= B <= %d]" % self.n_beams)
            S, k, n_beams = src.shape
            ami = np.asarray(angle_min_inc, np.float32)
            if ami.shape != (S, k, 2):
                raise LsdError(LSD_ERR_INVALID, "angle_min_inc must be [n_robots, k, 2]")
        od = np.ascontiguousarray(odom, np.float64).reshape(S, k, 3)
        nf = self._n_frames(n_frames, S, k)
        take = (np.arange(k)[None, :] < nf[:, None]).astype(np.int32)        # slots past a robot's frames: nothing to scan
        n = S * k
        self._staging(n)
        b = lambda a: a.reshape(-1).view(np.uint8)
        if ranges is None:                                                   # the frames (16-byte pairs) first
            host_in = np.concatenate([b(src), b(od), b(take)])
            d_src = self._in.data_ptr()
            d_od, d_ami = d_src + n * 16 * self.n_beams, None
        else:                                                                # the doubles first, then the floats
            host_in = np.concatenate([b(od), b(src), b(ami), b(take)])
            d_od = self._in.data_ptr()
            d_src = d_od + n * 24
            d_ami = d_src + src.nbytes
        d_take = self._in.data_ptr() + len(host_in) - 4 * n
        self._in[:len(host_in)].copy_(torch.from_numpy(host_in))
        b_st, b_rp = self._enqueue(S, k, nf, d_src if ranges is None else None, None if ranges is None else d_src, d_ami, n_beams, d_take, d_od)
        # the device-made maps: their line counts ride in the read-back
        live = [(i, pair.current) for i, pair in enumerate(self._pairs) if pair.current.n_host is None]
        end = n * self._OUT_B
        for j, (i, m) in enumerate(live):
            self._out[end + 4 * j:end + 4 * j + 4].view(torch.int32).copy_(m.count)
        out = self._out[:end + 4 * len(live)].cpu().numpy()                  # the tick's one synchronisation
        states = out[:b_st].view(FA_STATE_DTYPE).reshape(S, k)
        reports = out[b_st:b_st + b_rp].view(FA_REPORT_DTYPE).reshape(S, k)
        counts = out[b_st + b_rp:end].view(np.int32).reshape(2, n)
        if live:
            n_map = out[end:].view(np.int32)
            for j, (i, m) in enumerate(live):
                if n_map[j] < 0:
                    raise LsdError(LSD_ERR_INTERNAL, self._GAVE_UP % dict(i=i), partial=(states, reports))
            for j, (i, m) in enumerate(live):
                if n_map[j] > m.lines_cap:
                    raise LsdError(LSD_ERR_CAPACITY, self._OVER % dict(i=i, n=n_map[j], cap=m.lines_cap), partial=(states, reports))
        if (counts[0] > 360).any() or (counts[1] > self.pts_cap).any():
            raise LsdError(LSD_ERR_CAPACITY, load_library().lsd_strerror(LSD_ERR_CAPACITY).decode(), partial=(states, reports))
        return states, reports

    def step_device(self, lidar=None, odom=None, n_frames=None, *, ranges=None, angle_min_inc=None):
        """step() for a caller whose scans are on the device, without an upload, a read-back or a synchronisation: everything is enqueued
        on the current torch stream.  Either lidar, a CUDA float64 tensor [S, k, n_beams, 2] of raw (range, angle) frames, or ranges, a CUDA
        float32 tensor [S, k, B <= n_beams] (n_beams: the constructor's, default 360; a shorter lidar pads its tail with +inf, see step) with angle_min_inc CUDA float32 [S, k, 2] (sensor_msgs/LaserScan: ranges[], angle_min,
        angle_increment; the angle of beam i is angle_min + i * angle_increment in single precision, as laserCallback computes it).
        Readings whose range is +inf are dropped on the device (-inf and NaN are kept, as the reference's `!= INFINITY` keeps them).
        odom: CUDA float64 [S, k, 3]; n_frames: as in step(), a HOST int array (when given, its take flags are one small asynchronous
        upload).  Returns CUDA tensors (states uint8 [S, k, 720], reports uint8 [S, k, 72], counts int32 [2, S * k]): views of the
        Localizer's own staging, valid until the next step*() call and, after the caller's synchronisation, readable as FA_STATE_DTYPE /
        FA_REPORT_DTYPE records (`.cpu().numpy().view(FA_STATE_DTYPE)`); counts are FeatureScan's line and pixel counts per slot, for the
        caller's own capacity check (more than 360 resp. pts_cap: the records are computed from the stored part).  Once the staging and the
        context's workspace have their size (the first call, or a larger S * k) nothing here waits for the device."""
        import torch
        if (lidar is None) == (ranges is None):
            raise LsdError(LSD_ERR_INVALID, "give either lidar or ranges")
        src = lidar if ranges is None else ranges
        want = torch.float64 if ranges is None else torch.float32
        tensors = [("lidar" if ranges is None else "ranges", src, want), ("odom", odom, torch.float64)]
        if ranges is not None:
            tensors.append(("angle_min_inc", angle_min_inc, torch.float32))
        for name, t, dt in tensors:
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dt:
                raise LsdError(LSD_ERR_INVALID, "%s must be a CUDA %s tensor" % (name, str(dt).replace("torch.", "")))
        S = self.n_robots
        k = src.shape[1] if src.dim() >= 2 else 0
        if ranges is None:
            if tuple(src.shape) != (S, k, self.n_beams, 2) or k < 1:
                raise LsdError(LSD_ERR_INVALID, "lidar must be [n_robots, k >= 1, %d, 2]" % self.n_beams)
            n_beams = self.n_beams
        else:
            n_beams = src.shape[2] if src.dim() == 3 else 0
            if tuple(src.shape) != (S, k, n_beams) or k < 1 or not 1 <= n_beams <= self.n_beams:
                raise LsdError(LSD_ERR_INVALID, "ranges must be [n_robots, k >= 1, 1 <= B <= %d]" % self.n_beams)
            if tuple(angle_min_inc.shape) != (S, k, 2):
                raise LsdError(LSD_ERR_INVALID, "angle_min_inc must be [n_robots, k, 2]")
        if tuple(odom.shape) != (S, k, 3):
            raise LsdError(LSD_ERR_INVALID, "odom must be [n_robots, k, 3]")
        nf = self._n_frames(n_frames, S, k)
        self._staging(S * k)
        take = None
        if n_frames is not None:
            # pinned, so the copy does not wait for the stream; torch's host allocator keeps the block until the copy has run
            take = torch.from_numpy((np.arange(k)[None, :] < nf[:, None]).astype(np.int32)).pin_memory().to("cuda", non_blocking=True)
        src, od = src.contiguous(), odom.contiguous()
        ami = None if ranges is None else angle_min_inc.contiguous()
        self._held = (src, od, ami, take)                                    # the launches read them: alive until the next tick
        b_st, b_rp = self._enqueue(S, k, nf, src.data_ptr() if ranges is None else None, None if ranges is None else src.data_ptr(),
                                   None if ami is None else ami.data_ptr(), n_beams, None if take is None else take.data_ptr(), od.data_ptr())
        n = S * k
        return (self._out[:b_st].view(S, k, -1), self._out[b_st:b_st + b_rp].view(S, k, -1),
                self._out[b_st + b_rp:n * self._OUT_B].view(torch.int32).view(2, n))


class Localizer(_Ticks):
    """The laser side of the ROS node (laserCallback, LSD/main_on_linux.cpp:48-90) for n_robots robots against one map, with the replay
    driver's frame loop (LSD/main_on_windows.cpp:80-180) carried from call to call: each step() advances every robot by its frames of the
    tick (FeatureScan, FeatureAssociation, the UKF and the angle bookkeeping on the device, one stream), and the result is the same, bit for
    bit, as one lsd_localize call over each robot's whole log.  The map (its cache and lines), the robots' carries (FA_CARRY_DTYPE) and the
    FeatureScan staging live on the device (torch).  The map side (mapCallback, :97-134) is set_map from host arrays or set_map_device
    from a grid on the device: the Localizer holds two map slots, a new map is made in the one the ticks are not reading -- on a side
    stream if the caller wants -- and handed over through events, so ticks keep running on the old map meanwhile.  Like the context it
    uses, a Localizer serves one thread at a time, and its ticks one stream at a time.  The code is _Ticks': the methods here pass map
    index 0 to it, and the ticks go through the single-map entries.
    n_beams (default 360, the reference's lidar; 1 .. LSD_SCAN_MAX_LEN = 4096): the readings per scan of the robots' lidar -- 1081 for a
    UTM-30LX or an LMS1xx, 1141 for an LMS5xx, up to 3200 for an RPLidar S.  Above 1024 the context's scan capacity is raised to it
    (Context.set_scan_capacity) and FeatureScan runs on its long kernel; the line records stay at 360 per scan."""

    def __init__(self, map_cache, map_lines, map_param, n_robots=1, odom0=(0.0, 0.0, 0.0), ctx=None, pts_cap=8192, n_beams=360):
        super().__init__(ctx, n_robots, pts_cap, n_beams=n_beams)
        self._set_map(0, map_cache, map_lines, map_param, False)
        self.reset(range(self.n_robots), odom0)

    @classmethod
    def from_occupancy_grid(cls, data, oriMapCol, oriMapRow, mapResol, mapOriX, mapOriY, n_robots=1, odom0=(0.0, 0.0, 0.0), ctx=None,
                            n_beams=360):
        """A Localizer on the map mapCallback makes of an OccupancyGrid (map_param from the map metadata, mapParamCallback :92-99)."""
        _check_n_beams(n_beams)                                              # (before the map is made)
        _, mapCache, LSD = mapCallback(data, oriMapCol, oriMapRow, mapResol, ctx=ctx)
        return cls(mapCache, LSD.linesInfo, (oriMapCol, oriMapRow, mapResol, mapOriX, mapOriY), n_robots, odom0, ctx, n_beams=n_beams)

    @property
    def map_param(self):
        """(oriMapCol, oriMapRow, mapResol, mapOriX, mapOriY) of the map the next tick reads: set_map's default."""
        return self._pairs[0].current.map_param

    def _rebase_key(self, i):
        return None, 0                                                       # every robot

    def _carve(self, i):
        import torch
        S, cur, d_out = self.n_robots, self._pairs[0].current, self._out.data_ptr()
        self.ctx.enqueue_localize_resume_live_map_device(cur.mc.data_ptr(), cur.cols, cur.rows, cur.lines.data_ptr(), self._caps[0],
                                                         cur.count.data_ptr(), S, 1, np.zeros(S, np.int32), self._lines.data_ptr(),
                                                         self._lens.data_ptr(), self._pts.data_ptr(), self.pts_cap, self._lens.data_ptr(),
                                                         self._lp.data_ptr(), self._in.data_ptr(), cur.map_param[2], self._carry.data_ptr(),
                                                         d_out, d_out, torch.cuda.current_stream().cuda_stream)

    def set_map(self, map_cache, map_lines, map_param=None, rebase=False):
        """A new map (mapCallback) from host arrays or tensors (map_param: default, the one in use); the robots keep their carries.  It
        is copied, on the current torch stream, into the map slot the ticks are not reading, and the ticks after the call read that
        slot: the hand-over of set_map_device, with the line count known to the host, so a host-made and a device-made map can
        alternate.  rebase: as set_map_device's."""
        self._set_map(0, map_cache, map_lines, self.map_param if map_param is None else map_param, rebase)

    def reserve_map(self, cols, rows, lines_cap=512):
        """Sizes everything a set_map_device of a cols x rows grid (or a smaller one) and the ticks after it need: both map slots
        (lines_cap records each: from now on a device-made map keeps its first lines_cap lines and the ticks' workspace is sized for
        lines_cap x 360 pairs per robot), the map side's context (lsd_reserve_map_update for the largest geometry reserved so far) and
        the ticks' workspace.  A set-up call: it waits for the device.  After it neither set_map_device nor the ticks wait for the
        device or allocate."""
        self._reserve_map(0, cols, rows, lines_cap)

    def set_map_device(self, d_grid, oriMapCol, oriMapRow, mapResol, mapOriX, mapOriY, stream=None):
        """mapCallback for an OccupancyGrid that is already on the device, without a host round trip: d_grid is a CUDA int8 tensor of
        oriMapRow * oriMapCol cells (flat, or [rows, cols]), ready on `stream` (a torch.cuda.Stream; default: the current one).  The
        whole callback (lsd_enqueue_map_update_device: cells, mapCache with the callback's z_occ_max_dis = 2, the detector) is enqueued
        on `stream` into the map slot the ticks are NOT reading, behind an event recorded after the last tick that read that slot, and
        an event is recorded behind it.  Ticks enqueued before this call keep the old map; the first tick after it puts its own stream
        behind that event and reads the new slot -- the line count on the device (map_counts), map_param from this call's arguments.
        Nothing here waits for the device once reserve_map covers the geometry; a larger grid, or more lines than the slot holds, makes
        the slot grow first, which waits on the host for the ticks that still read it and for its last update.  A map with more than
        lines_cap lines (reserve_map; default 512) keeps its first lines_cap: step() then raises LSD_ERR_CAPACITY, a step_device
        caller checks map_counts.
        The re-base: the carries are in pixels of the map they were made on, so a map that comes back with another origin or resolution
        (a SLAM map that grew) leaves every lastPose off by the shift -- beyond maxEstiDist the track is lost.  This method's parameter
        list is fixed, so it has no keyword for it: set the attribute rebase_on_hand_over = True (set_map, and FleetLocalizer's set_map
        and set_map_device, also take rebase=True for one call).  With it, and a map_param that differs from the one the ticks were
        using in mapResol, mapOriX or mapOriY, every robot's carry is moved to the new frame (lsd_enqueue_fa_carry_rebase_device: the
        pose in metres is kept up to rounding; a robot without a pose is left alone) by the first tick after this call, on that tick's
        stream, in front of its launches: ticks enqueued earlier read the old map with old-frame carries, this tick and later ones the
        new map with new-frame carries, and nothing waits on the host.  Two hand-overs without a tick between them compose (the
        earliest `from`, the latest `to`); reset, carries and a carries assignment enqueue a pending re-base first.  The default,
        rebase_on_hand_over = False, leaves the carries alone.  Only the origin's position and the resolution are followed: a map
        frame that rotates is not."""
        self._set_map_device(0, d_grid, oriMapCol, oriMapRow, mapResol, mapOriX, mapOriY, stream, False)

    @property
    def map_counts(self):
        """The line count of the map the next tick reads: a CUDA int32 tensor of one element, valid once the update that makes the map
        has run (the caller's synchronisation).  Above lines_cap: the ticks use the first lines_cap lines; -1: the detector gave the map
        up and the ticks see no map lines."""
        return self._pairs[0].current.count

    def integrate_last_tick(self, mapper):
        """Mapping with known poses: enqueues, on the stream of the last step / step_device and behind it, the integration into `mapper`
        (a GridMapper) of every frame of that tick, each at the state it produced -- the packed scans and the states are read from the
        tick's own staging, nothing is read back and nothing waits.  A frame whose state has no pose (a reset: x = -1) falls out by the
        mapper's "no pose" rule, a slot past a robot's n_frames holds an empty scan.  Call it before the next tick, which reuses the
        staging.  The poses are in pixels of the map the tick localised on: the mapper's mapResol / mapOriX / mapOriY are that map's.
        With mapper.publish_device() feeding set_map_device(grid, *mapper.map_param) the loop closes on the device."""
        self._integrate_last_tick(mapper, range(self.n_robots))

    def append_last_tick(self, graph, robot=0, track=None, append=None):
        """Keyframes of the last tick into a PoseGraph: on the tick's stream and behind it, the frames of `robot` are
        the candidates of graph.append_device, each at the state it produced (pitch 720), read from the tick's staging; nothing is read
        back and nothing waits.  track: the graph's track they continue (None: the robot's index).  Call it before the next tick."""
        self._append_last_tick(graph, robot, int(robot) if track is None else track, append)

    def screen_and_integrate_last_tick(self, mapper, ray=None, d_grid=None):
        """integrate_last_tick with the ray-casting stage in front (GridMapper.screen_and_integrate_device): on the last
        tick's stream and behind the tick, every frame of the tick is cast through the grid (d_grid, or None: the mapper's planes
        published now) from the state it produced (pitch 720), and its screened scan is integrated at its summary record.  Nothing is
        read back and nothing waits.  Returns (rays, sums): CUDA uint8 tensors [n_robots * k, n_beams, 32] (GRID_RAY_DTYPE) and
        [n_robots * k, 64] (GRID_RAY_SUM_DTYPE); slot s * k + t is frame t of robot s."""
        if self._last_tick is None:
            raise LsdError(LSD_ERR_INVALID, "no tick has been enqueued yet")
        if not isinstance(mapper, GridMapper):
            raise LsdError(LSD_ERR_INVALID, "mapper must be a GridMapper")
        S, k, ts, _ = self._last_tick
        return mapper._screen_and_integrate(self.ctx, self._scans.data_ptr(), self._lens.data_ptr(), S * k, self.n_beams, self._out.data_ptr(),
                                            FA_STATE_DTYPE.itemsize, ray, d_grid, ts)

    def refine_and_integrate_last_tick(self, mapper, search=None, refresh=True, smear=None, block=0, response=None, integrate_at="match",
                                       correct=None):
        """integrate_last_tick with the correlative match in front (GridMapper.match_and_integrate_device): on the last
        tick's stream and behind the tick, the mapper's lookup plane is refreshed (refresh=False: kept as it is), every frame of the tick is
        matched on it around the state it produced (pitch 720), and integrated at the record's pose.  Nothing is read back and nothing
        waits.  Returns the records, a CUDA uint8 tensor [n_robots * k, 56] (GRID_MATCH_DTYPE; slot s * k + t is frame t of robot s).
        block = 2..16: the same records by the coarse-to-fine search.  response (grid_response()) given: the response
        stage behind the match, and (records, response records: a CUDA uint8 tensor [n_robots * k, 192],
        GRID_RESPONSE_DTYPE) is returned; then integrate_at="response" integrates at the refined poses instead of the records'.
        correct (fa_correct(); True: its defaults) given -- it needs response, else LSD_ERR_INVALID --: correct_last_tick behind the
        response stage, and its reports are returned last in the tuple.  None, the default, enqueues nothing more."""
        return self._refine_and_integrate_last_tick(mapper, None, (None, 0), search, refresh, smear, block, response, integrate_at, correct)

    def locate_last_tick(self, mapper, locate=None, refresh=True, smear=None, stats=False, tight=None):
        """Global localisation of the last tick's scans (GridMapper.locate_device): on the last tick's stream and behind
        the tick, every frame slot of the tick is located on `mapper`'s grid from the tick's ingested scans alone -- the states the tick
        produced play no part, so a robot whose tick ended in a reset, or one that has no pose yet, is located as well.  Nothing is read
        back and nothing waits.  Returns the records, a CUDA uint8 tensor [n_robots * k, 64] (GRID_LOCATE_DTYPE; slot s * k + t is frame t
        of robot s; a slot past a robot's n_frames holds an empty scan: GRID_LOCATE_EMPTY).  This call only reports: no carry is written,
        and every slot is searched, the robots that know where they are included.  relocate_last_tick locates the lost robots alone and
        writes the poses into their carries.  tight: GridMapper.locate_device's (the statistics are then [n, 128])."""
        if self._last_tick is None:
            raise LsdError(LSD_ERR_INVALID, "no tick has been enqueued yet")
        if not isinstance(mapper, GridMapper):
            raise LsdError(LSD_ERR_INVALID, "mapper must be a GridMapper")
        S, k, ts, _ = self._last_tick
        return mapper._enqueue_locate(self.ctx, self._scans.data_ptr(), self._lens.data_ptr(), S * k, self.n_beams, locate, refresh, smear, stats,
                                      ts, tight)

    def relocate_last_tick(self, mapper, locate=None, seed=None, max_lost=1, refresh=True, smear=None, response=None, search=None, stats=False,
                           tight=None):
        """Relocalisation of the robots the last tick left without a pose, on the last tick's stream and behind the tick,
        in this order: the lost robots -- a carry without a pose whose tick had a scan -- are gathered in ascending index, the first
        max_lost of them with their scans packed into a batch of max_lost rows (lsd_enqueue_fa_lost_gather_device); that batch is located
        on `mapper`'s grid as locate_device locates (locate, refresh, smear, stats: its arguments), so the launches and the workspace
        follow max_lost and not the fleet; with response (grid_response(); True: its defaults) a match of zero window at the located poses
        -- the response stage reads a match record, which a locate record is not -- and the response stage behind it (search: its
        ang_step and acceptance thresholds; the window is forced to zero); then the accepted, unambiguous poses are written into the
        carries (lsd_enqueue_fa_carry_seed_device; seed: fa_seed()) with the loop's angle bookkeeping replaced by the one offset a first
        frame at that pose would push, so the NEXT tick tracks from the located pose.  Nothing is read back and nothing waits.  Returns
        CUDA tensors (pick int32 [max_lost]: the slot s * k + t gathered into each row, -1 for an unused row; n_lost int32 [2]: the robots
        lost -- it may exceed max_lost: call again, the seeded ones are no longer lost -- and the robots gathered; the locate records
        uint8 [max_lost, 64]; with stats their statistics [max_lost, 48]; with response the response records [max_lost, 192]; the seed
        reports uint8 [max_lost, 48], FA_SEED_DTYPE).  tight: GridMapper.locate_device's -- the locate of the chain under the tight rule
        (DESIGN.md 8.1.14): a robot whose search overflows is not seeded, and the tight rule overflows less; the statistics are then
        [max_lost, 128]."""
        return self._relocate_last_tick(mapper, (None, 0), locate, seed, max_lost, refresh, smear, response, search, stats, tight=tight)

    def correct_last_tick(self, responses, correct=None):
        """The grid match response fused into the robots' carries (lsd_enqueue_fa_carry_correct_device): a measurement
        update of each robot's 9-state filter with its response record as the measurement, weighed by the record's covariance (correct:
        fa_correct(); None: its defaults), so that the NEXT tick starts from the corrected pose.  responses: the response records of the last
        tick's slots, a CUDA uint8 tensor [n_robots * k, 192], as refine_and_integrate_last_tick(response=...) returns them for that tick.
        On the last tick's stream and behind the tick; the poses are the tick's states (pitch 720), the carries the localiser's; nothing is
        read back or waits.  Per robot the slot whose state equals the carry's pose, byte for byte, is the one fused -- the last frame the
        tick took (with k > 1 the earlier frames' responses are not fused: the loop has consumed their states) --, so a second call on the
        same tick finds no such slot and changes nothing (FA_CORRECT_STALE).  Returns the reports: a CUDA uint8 tensor [n_robots, 48]
        (FA_CORRECT_DTYPE: the innovation, its squared Mahalanobis distance, det S, the slot and one FA_CORRECT_* flag)."""
        return self._correct_last_tick(responses, correct, (None, 0))

    def _feature_scan(self, n, k, d_scans, d_lens, d_n_lines, d_n_pts, stream):
        cx, m = self.ctx, self._pairs[0].current
        cx._chk(cx.L.lsd_enqueue_feature_scan_batch_device(cx.h, d_scans, d_lens, n, self.n_beams, _map_param(m.map_param), rdp_leastPoint, rdp_threLine,
                                                           rdp_leastDist, self._lines.data_ptr(), d_n_lines, self._pts.data_ptr(), self.pts_cap,
                                                           d_n_pts, self._lp.data_ptr(), self._sz.data_ptr(), stream))

    def _loop(self, S, k, nf, d_n_lines, d_n_pts, d_od, d_states, d_reports, stream):
        m = self._pairs[0].current
        tail = (S, k, nf, self._lines.data_ptr(), d_n_lines, self._pts.data_ptr(), self.pts_cap, d_n_pts, self._lp.data_ptr(), d_od, m.map_param[2],
                self._carry.data_ptr(), d_states, d_reports, stream)
        if m.n_host is not None:
            self.ctx.enqueue_localize_resume_device(m.mc.data_ptr(), m.cols, m.rows, m.lines.data_ptr(), m.n_host, *tail)
        else:                                                                # a map made on the device: so is its line count
            self.ctx.enqueue_localize_resume_live_map_device(m.mc.data_ptr(), m.cols, m.rows, m.lines.data_ptr(), m.lines_cap, m.count.data_ptr(), *tail)


def fleet_map_ids(map_ids, n_maps, count=None):
    """Map ids as the fleet entries read them: int32 [count], each a map of the table (0..n_maps-1) or -1 (the robot sits out)."""
    ids = np.ascontiguousarray(map_ids, np.int32).reshape(-1)
    if count is not None and len(ids) != count:
        raise LsdError(LSD_ERR_INVALID, "one map id per robot")
    if ((ids < -1) | (ids >= n_maps)).any():
        raise LsdError(LSD_ERR_INVALID, "a map id is 0..%d, or -1 for a robot that sits out" % (n_maps - 1))
    return ids


class FleetLocalizer(_Ticks):
    """Localizer for a fleet on several maps: every robot is ticked against the map its id names, all of them in ONE tick (one ingest,
    one FeatureScan launch and one set of FeatureAssociation launches per frame index: lsd_enqueue_feature_scan_maps_device with
    scans_per_seq = k, lsd_enqueue_localize_resume_maps_device), and each gets, bit for bit, what a Localizer on its map alone gives
    it.  maps: a list of (map_cache, map_lines, map_param) host arrays, one per map id (at most LSD_MAX_MAPS); map_of: one id per robot
    -- this sets n_robots --, or -1 for a robot that sits out (parked, between floors): its carry stays as it is and its slots of a
    tick's results stay zero.  The ids live on the device: assign() rewrites them on the current stream.  step, step_device, reset and
    carries are Localizer's (the same code, _Ticks').  So is the map side, per map id: every map has two slots, set_map(i, ...) from
    host arrays or set_map_device(i, ...) from a grid on the device makes the new map in the slot the ticks are not reading -- on a side
    stream if the caller wants -- and hands it over through events, so the ticks keep running on the old map meanwhile;
    reserve_map(i, ...) sizes what that needs.  One map-side context serves all maps: updates of different maps on different streams
    serialise on the device (lsd_enqueue_map_update_device orders itself behind the context's previous run with an event), never on
    the host.  Like the context it uses, a FleetLocalizer serves one thread at a time, and its ticks one stream at a time.
    n_beams: as Localizer's, one value for the fleet.  A fleet with mixed lidars uses the largest; a robot with fewer readings pads each
    scan at the tail with +inf ranges, which the ingest drops, so its scan is exactly the shorter one (in the LaserScan layout the kept
    beams' angles, angle_min + i * angle_increment, do not depend on the padded length)."""

    _GAVE_UP = "map %(i)d: the detector gave the map up (count -1): the tick saw no map lines"
    _OVER = "map %(i)d has %(n)d lines, its slots hold %(cap)d (reserve_map): the tick used the first %(cap)d"

    def __init__(self, maps, map_of, odom0=(0.0, 0.0, 0.0), ctx=None, pts_cap=8192, n_beams=360):
        import torch
        maps = list(maps)
        if not maps:
            raise LsdError(LSD_ERR_INVALID, "at least one map")
        if len(maps) > LSD_MAX_MAPS:
            raise LsdError(LSD_ERR_UNSUPPORTED, "more than LSD_MAX_MAPS = %d maps" % LSD_MAX_MAPS)
        ids = fleet_map_ids(map_of, len(maps))
        if not len(ids):
            raise LsdError(LSD_ERR_INVALID, "at least one robot")
        super().__init__(ctx, len(ids), pts_cap, len(maps), n_beams=n_beams)
        self._table = np.zeros(len(maps), MAP_REF_DTYPE)                     # what the *_maps entries take: record i names map i's current slot
        self._mask = None
        for i, m in enumerate(maps):
            self.set_map(i, *m)
        self._map_of = torch.from_numpy(ids).cuda()
        self._map_of_host = ids.copy()                                       # the ids as enqueued so far (integrate_last_tick's filter)
        self.reset(range(self.n_robots), odom0)

    @property
    def n_maps(self):
        return len(self._table)

    @property
    def map_of(self):
        """The robots' map ids, int32 [n_robots] on the host (a read-back)."""
        return self._map_of.cpu().numpy()

    def _map_id(self, i):
        i = int(i)
        if not 0 <= i < len(self._table):
            raise LsdError(LSD_ERR_INVALID, "map %d of %d" % (i, len(self._table)))
        return i

    def _rebase_key(self, i):
        return self._map_of.data_ptr(), i                                    # the robots on map i

    def _map_changed(self, i):
        m = self._pairs[i].current                                           # a device-made map: its count on the device, lines_cap as the capacity
        self._table[i] = map_ref(m.mc.data_ptr(), m.cols, m.rows, m.lines.data_ptr(), m.lines_cap if m.n_host is None else m.n_host, m.map_param,
                                 m.count.data_ptr() if m.n_host is None else 0)

    def _carve(self, i):
        import torch
        S, d_out = self.n_robots, self._out.data_ptr()
        tab = self._table.copy()
        tab[i]["n_map"] = max(max(self._caps), int(tab["n_map"].max()))      # the table's largest capacity (no frame: no record of it is read)
        self.ctx.enqueue_localize_resume_maps_device(tab, self._map_of.data_ptr(), S, 1, np.zeros(S, np.int32), self._lines.data_ptr(),
                                                     self._lens.data_ptr(), self._pts.data_ptr(), self.pts_cap, self._lens.data_ptr(),
                                                     self._lp.data_ptr(), self._in.data_ptr(), self._carry.data_ptr(), d_out, d_out,
                                                     torch.cuda.current_stream().cuda_stream)

    def set_map(self, i, map_cache, map_lines, map_param, rebase=False):
        """Localizer.set_map for map i; the robots on it keep their carries, the robots on other maps are not affected."""
        self._set_map(self._map_id(i), map_cache, map_lines, map_param, rebase)

    def reserve_map(self, i, cols, rows, lines_cap=512):
        """Localizer.reserve_map for map i: both slots of map i, the one map-side context, and the ticks' workspace for the largest
        lines_cap and line count of the table."""
        self._reserve_map(self._map_id(i), cols, rows, lines_cap)

    def set_map_device(self, i, d_grid, oriMapCol, oriMapRow, mapResol, mapOriX, mapOriY, stream=None, rebase=False):
        """Localizer.set_map_device for map i: the whole map callback (lsd_enqueue_map_update_device) is enqueued on `stream` (a
        torch.cuda.Stream; default: the current one) into the slot of map i that the ticks are NOT reading, behind an event recorded
        after the last tick that read that slot, and table record i is rewritten: the slot's cache and lines, its count on the device,
        lines_cap (reserve_map; default 512) as the capacity, the new geometry.  Ticks enqueued before the call keep the old map; the
        first tick after it puts its own stream behind the update.  The robots on other maps are not affected.  Nothing here waits for
        the device once reserve_map(i, ...) covers the geometry.  A map with more than lines_cap lines keeps its first lines_cap:
        step() then raises LSD_ERR_CAPACITY and names the map, a step_device caller checks map_counts.
        rebase=True: when the new map_param differs from the one the ticks were using for map i in mapResol, mapOriX or mapOriY, the
        carries of the robots that are on map i when the next tick runs are moved to the new frame by that tick, in front of its
        launches (Localizer.set_map_device; lsd_enqueue_fa_carry_rebase_device with d_key = the robots' map ids, key = i)."""
        self._set_map_device(self._map_id(i), d_grid, oriMapCol, oriMapRow, mapResol, mapOriX, mapOriY, stream, rebase)

    @property
    def map_counts(self):
        """Per map id, the line count of the map the next tick reads: a list of CUDA int32 tensors of one element, with
        Localizer.map_counts' conventions (valid once the update that makes the map has run; above the map's lines_cap: the ticks use
        the first lines_cap lines; -1: the detector gave the map up and the ticks see no map lines)."""
        return [pair.current.count for pair in self._pairs]

    def assign(self, robots, map_ids):
        """Moves the given robots to the given maps (one id each, or one for all; -1: the robot sits out from now on): the ids are
        rewritten on the device, on the current torch stream, without waiting for it (a pending re-base is enqueued first: it is for
        the robots that were on its map).  The carries are NOT touched, and a carry is in the pixel frame of the map it was made on:
        after a move follow with rebase(robots, from_map, to_map) if the two maps share a world frame, else with reset(robots, odom0,
        state)."""
        import torch
        idx = np.ascontiguousarray([int(r) for r in robots], np.int64)
        if not len(idx):
            return
        if ((idx < 0) | (idx >= self.n_robots)).any():
            raise LsdError(LSD_ERR_INVALID, "a robot is 0..%d" % (self.n_robots - 1))
        ids = np.asarray(map_ids, np.int32).reshape(-1)
        ids = fleet_map_ids(np.repeat(ids, len(idx)) if len(ids) == 1 else ids, len(self._table), len(idx))
        self._flush_rebase()
        # pinned, so the copies do not wait for the stream (as the take flags of step_device)
        up = lambda a: torch.from_numpy(a).pin_memory().to("cuda", non_blocking=True)
        self._map_of.index_copy_(0, up(idx), up(ids))
        self._map_of_host[idx] = ids

    def rebase(self, robots, from_map, to_map):
        """Moves the given robots' carries from the pixel frame of map from_map to that of map to_map (the map_param the next tick
        uses for each), on the current torch stream, without waiting for it: lsd_enqueue_fa_carry_rebase_device with a small device
        mask as the key.  The use: after assign() has moved robots between maps of ONE site that share a world frame -- two halls, an
        annex, the same floor at two resolutions -- they keep tracking where a reset would start them over; the pose in metres is kept
        up to rounding, a robot without a pose is left alone.  Maps in unrelated world frames (or frames that are rotated against each
        other: only the origin's position and the resolution are followed) still need reset."""
        import torch
        idx = np.ascontiguousarray([int(r) for r in robots], np.int64)
        a, b = self._map_id(from_map), self._map_id(to_map)
        if ((idx < 0) | (idx >= self.n_robots)).any():
            raise LsdError(LSD_ERR_INVALID, "a robot is 0..%d" % (self.n_robots - 1))
        f, t = map_frame(self._pairs[a].current.map_param), map_frame(self._pairs[b].current.map_param)
        if not len(idx):
            return
        self._flush_rebase()
        mask = np.zeros(self.n_robots, np.int32)
        mask[idx] = 1
        if self._mask is None:
            self._mask = torch.zeros(self.n_robots, dtype=torch.int32, device="cuda")
        self._mask.copy_(torch.from_numpy(mask).pin_memory(), non_blocking=True)
        self.ctx.enqueue_fa_carry_rebase_device(self._carry.data_ptr(), self.n_robots, self._mask.data_ptr(), 1, f, t,
                                                torch.cuda.current_stream().cuda_stream)

    def _tick_robots(self):
        return self._map_of_host.copy()

    def integrate_last_tick(self, mapper, map_id):
        """Localizer.integrate_last_tick for the robots that were on map `map_id` when the last tick was enqueued (the ids as
        assign() had left them by then; robots on other maps and robots that sat out are not touched): one launch per run of
        neighbouring robots.  The mapper's frame is that map's."""
        i = self._map_id(map_id)
        if self._last_tick is None:
            raise LsdError(LSD_ERR_INVALID, "no tick has been enqueued yet")
        self._integrate_last_tick(mapper, np.flatnonzero(self._last_tick[3] == i))

    def append_last_tick(self, graph, map_id, robot, track=None, append=None):
        """Localizer.append_last_tick for `robot`, which was on map `map_id` when the last tick was enqueued (LsdError otherwise): a fleet
        has one graph per map, and the robot's poses are in that map's pixels.  track: None, the robot's index -- the graph needs that
        many tracks."""
        i = self._map_id(map_id)
        if self._last_tick is None:
            raise LsdError(LSD_ERR_INVALID, "no tick has been enqueued yet")
        if not 0 <= int(robot) < self.n_robots or self._last_tick[3][int(robot)] != i:
            raise LsdError(LSD_ERR_INVALID, "robot %r was not on map %r in the last tick" % (robot, map_id))
        self._append_last_tick(graph, robot, int(robot) if track is None else track, append)

    def refine_and_integrate_last_tick(self, mapper, map_id, search=None, refresh=True, smear=None, block=0, response=None, integrate_at="match",
                                       correct=None):
        """Localizer.refine_and_integrate_last_tick for the robots that were on map `map_id` when the last tick was enqueued, as
        integrate_last_tick(mapper, map_id) selects them: the lookup plane is refreshed once, then match, response and integration are
        enqueued per run of neighbouring robots.  The returned tensors cover all n_robots * k slots (the reports: n_robots); the slots of
        the other robots are zero bytes.  correct given: the correction reads the robots' map ids on the device (d_key = the ids, key =
        map_id), so a robot an assign() has moved off the map since keeps its carry; the other robots' carries keep every byte."""
        i = self._map_id(map_id)
        if self._last_tick is None:
            raise LsdError(LSD_ERR_INVALID, "no tick has been enqueued yet")
        return self._refine_and_integrate_last_tick(mapper, np.flatnonzero(self._last_tick[3] == i), (self._map_of.data_ptr(), i), search,
                                                    refresh, smear, block, response, integrate_at, correct)

    def locate_last_tick(self, mapper, map_id, locate=None, max_lost=1, refresh=True, smear=None, stats=False, tight=None):
        """Global localisation of the LOST robots on map `map_id` from the last tick's scans, without writing a carry: relocate_last_tick's
        gather and locate alone.  The robots' map ids are read on the device (d_key = the ids, key = map_id), so the call stays right
        behind an assign() on the stream; there is no host-side selection as integrate_last_tick makes one, and hence no locate of every
        slot as Localizer.locate_last_tick runs it -- a robot with a pose has its states, and GridMapper.locate_device takes any scans a
        caller holds.  Returns CUDA tensors (pick int32 [max_lost], n_lost int32 [2], the locate records uint8 [max_lost, 64]; with stats
        their statistics [max_lost, 48]); row j belongs to slot pick[j].  tight: GridMapper.locate_device's (statistics [max_lost, 128])."""
        return self._relocate_last_tick(mapper, (self._map_of.data_ptr(), self._map_id(map_id)), locate, None, max_lost, refresh, smear, None, None,
                                        stats, write=False, tight=tight)

    def relocate_last_tick(self, mapper, map_id, locate=None, seed=None, max_lost=1, refresh=True, smear=None, response=None, search=None,
                           stats=False, tight=None):
        """Localizer.relocate_last_tick for the lost robots on map `map_id`, read on the device when the kernels run (d_key = the robots' map
        ids, key = map_id): right behind an assign() on the stream, and the robots on other maps keep every byte of their carries.  The
        mapper's frame is that map's.  tight: Localizer.relocate_last_tick's."""
        return self._relocate_last_tick(mapper, (self._map_of.data_ptr(), self._map_id(map_id)), locate, seed, max_lost, refresh, smear, response,
                                        search, stats, tight=tight)

    def correct_last_tick(self, responses, map_id, correct=None):
        """Localizer.correct_last_tick for the robots on map `map_id`, read on the device when the kernel runs (d_key = the robots' map ids,
        key = map_id): responses covers all n_robots * k slots, as refine_and_integrate_last_tick(mapper, map_id, response=...) returns
        them; a robot on another map keeps its carry and its report is zero bytes."""
        return self._correct_last_tick(responses, correct, (self._map_of.data_ptr(), self._map_id(map_id)))

    def _feature_scan(self, n, k, d_scans, d_lens, d_n_lines, d_n_pts, stream):
        self.ctx.enqueue_feature_scan_maps_device(d_scans, d_lens, n, self.n_beams, self._table, self._map_of.data_ptr(), k, self._lines.data_ptr(), d_n_lines,
                                                  self._pts.data_ptr(), self.pts_cap, d_n_pts, self._lp.data_ptr(), self._sz.data_ptr(), stream=stream)

    def _loop(self, S, k, nf, d_n_lines, d_n_pts, d_od, d_states, d_reports, stream):
        self.ctx.enqueue_localize_resume_maps_device(self._table, self._map_of.data_ptr(), S, k, nf, self._lines.data_ptr(), d_n_lines,
                                                     self._pts.data_ptr(), self.pts_cap, d_n_pts, self._lp.data_ptr(), d_od, self._carry.data_ptr(),
                                                     d_states, d_reports, stream)


def mapCallback(data, oriMapCol, oriMapRow, mapResol, ctx=None):
    """The ROS node's map callback (LSD/main_on_linux.cpp:97-135): OccupancyGrid cells -> mapValue -> mapCache (with
    the callback's z_occ_max_dis = 2, :126-127) and the LSD result.  Returns (mapValue as rewritten by the LSD call,
    mapCache, structLSD)."""
    cx = ctx or default_context()
    grid = np.ascontiguousarray(np.asarray(data, np.int8).reshape(oriMapRow, oriMapCol))
    mapValue = cx.occupancy_to_map(grid)
    mapCache = cx.map_cache(mapValue, mapResol, 2.0)
    LSD = myLineSegmentDetector(mapValue, oriMapCol, oriMapRow, lsd_sca, lsd_sig, lsd_angThre, lsd_denThre, pseBin, ctx=cx)
    return mapValue, mapCache, LSD


def mapCallback_device(d_grid, oriMapCol, oriMapRow, mapResol, ctx=None, stream=None, max_lines=8192):
    """mapCallback for an OccupancyGrid that is already on the device (a CUDA int8 tensor of oriMapRow * oriMapCol cells, flat or
    [rows, cols]), as one enqueue (lsd_enqueue_map_update_device) on `stream` (a torch.cuda.Stream; default: the current one), without
    a synchronisation.  Returns CUDA tensors (map uint8 [rows, cols]: mapValue as the LSD call leaves it; map_cache float64 [rows,
    cols]; lines uint8 [max_lines, 80]: LINE_DTYPE records, the first min(count, max_lines) valid; count int32 [1]: len_linesInfo, above
    max_lines on overflow, -1 if the detector gave the map up; line_im uint8 [rows, cols]), readable after the caller's synchronisation."""
    import torch
    cx = ctx or default_context()
    cols, rows = int(oriMapCol), int(oriMapRow)
    grid = _occupancy_grid(d_grid, cols, rows, cx.device)
    stream = _cuda_stream(stream)
    with torch.cuda.stream(stream):                                          # (the outputs belong to the stream that writes them)
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=grid.device)
        m, mc, li = e((rows, cols), torch.uint8), e((rows, cols), torch.float64), e((rows, cols), torch.uint8)
        lines, count = e((int(max_lines), 80), torch.uint8), e((1,), torch.int32)
    cx.enqueue_map_update_device(grid.data_ptr(), cols, rows, float(mapResol), 2.0, m.data_ptr(), mc.data_ptr(), lines.data_ptr(), int(max_lines),
                                 count.data_ptr(), li.data_ptr(), None, stream.cuda_stream)
    grid.record_stream(stream)
    return m, mc, lines, count, li


def runLSD(MapGray, oriMapCol=None, oriMapRow=None, sca=lsd_sca, sig=lsd_sig, angThre=lsd_angThre,
           denThre=lsd_denThre, pseBin=pseBin, ctx=None):
    """`runLSD` is the name BASELINE.json's north_star uses; the reference has no such symbol
    (SURVEY section 0.1).  It is an alias of myLineSegmentDetector with the baseFunc.h defaults."""
    rows, cols = MapGray.shape
    return myLineSegmentDetector(MapGray, oriMapCol or cols, oriMapRow or rows, sca, sig, angThre, denThre, pseBin, ctx)
