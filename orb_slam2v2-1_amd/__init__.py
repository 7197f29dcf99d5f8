"""orb_slam2v2-1_amd — MI355X-native ORB front-end + Hamming matchers (HIP, gfx950).

Python-side binding of the C ABI in include/orbx.h (ctypes; no torch types cross the
boundary).  The classes mirror the reference's operator interface for this path:

  ORBextractor  <- include/ORBextractor.h:45-111   (ctor args, operator(), getters,
                                                     mvImagePyramid)
  ORBmatcher    <- include/ORBmatcher.h:37-102     (TH_LOW/TH_HIGH/HISTO_LENGTH,
                                                     DescriptorDistance, the hot Search*)
  compute_stereo_matches <- Frame::ComputeStereoMatches (src/Frame.cc:481-655)

There is NO CPU fallback: if the HIP library is missing or no GPU is usable the calls
raise OrbxError.  (The CPU oracle lives in /oracle and is test infrastructure only.)
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# The PRODUCT library (no test hooks), and the DEVELOPER build of the same sources (-DORBX_DEVELOPER: + the read-only stage hooks of
# include/orbx_dev.h, + the phase-stop / time-stamp option keys of the probes in tools/).  ORBX_LIB names another file for the first.
LIB_PATH = os.environ.get("ORBX_LIB") or os.path.join(_HERE, "lib", "liborbx_hip.so")
DEV_LIB_PATH = os.path.join(_HERE, "lib", "liborbx_hip_dev.so")
# extractors created while this is True come from the developer build (tests that look at intermediate stages: `hooks` fixture)
default_developer = False

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
MP_DTYPE = np.dtype([("in_view", "<i4"), ("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"),
                     ("level", "<i4"), ("view_cos", "<f4"), ("observations", "<i4")])
LASTPT_DTYPE = np.dtype([("has_mp", "<i4"), ("wx", "<f4"), ("wy", "<f4"), ("wz", "<f4"),
                         ("observations", "<i4"), ("octave", "<i4"), ("angle", "<f4")])
WINDOW_DTYPE = np.dtype([("valid", "<i4"), ("u", "<f4"), ("v", "<f4"), ("radius", "<f4"), ("min_level", "<i4"),
                         ("max_level", "<i4"), ("angle", "<f4"), ("blocks", "<i4"), ("ur_c", "<f4"), ("ur_tol", "<f4")])

# orbx_cloud_point_t: a point of a dense keyframe cloud (pcl::PointXYZRGBA's fields; "b" is channel 0 of the colour image)
CLOUD_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("b", "u1"), ("g", "u1"), ("r", "u1"), ("a", "u1")])

# orbx_octree_leaf_t: a leaf of the pruned occupancy octree (octomap key of its minimum corner, depth 1..16)
OCTREE_LEAF_DTYPE = np.dtype([("kx", "<u2"), ("ky", "<u2"), ("kz", "<u2"), ("depth", "<u2")])
# the reference's transform_trans * transform_rot_x * transform_rot_y (src/pointcloudmapping.cc:198-223): x' = z, y' = -x, z' = -y
OCTOMAP_AXIS_SWAP = np.array([[0, 0, 1, 0], [-1, 0, 0, 0], [0, -1, 0, 0], [0, 0, 0, 1]], np.float32)
# include/orbx.h: orbv_db_hit_t, one listed keyframe of a keyframe-database query (flags: bit 0 scored, bit 1 entered lScoreAndMatch)
# orbo_observation_t / orbo_worldpos_t / orbo_pose_info_t (pose_optimization*)
POSE_OBS_DTYPE = np.dtype([("valid", "<i4"), ("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("inv_sigma2", "<f4"),
                           ("wx", "<f4"), ("wy", "<f4"), ("wz", "<f4")])
POSE_WORLDPOS_DTYPE = np.dtype([("valid", "<i4"), ("wx", "<f4"), ("wy", "<f4"), ("wz", "<f4")])
POSE_INFO_DTYPE = np.dtype({"names": ["correspondences", "bad", "iterations", "trials", "rounds", "t", "q"],
                            "formats": ["<i4", "<i4", ("<i4", 4), ("<i4", 4), "<i4", ("<f8", 3), ("<f8", 4)],
                            "offsets": [0, 4, 8, 24, 40, 48, 72], "itemsize": 104})
# orbi_init_info_t (Initializer, initialize_device)
INIT_INFO_DTYPE = np.dtype([("SH", "<f4"), ("SF", "<f4"), ("RH", "<f4"), ("model", "<i4"), ("best_iteration", "<i4", (2,)),
                            ("inliers", "<i4", (2,)), ("best_good", "<i4"), ("second_good", "<i4"), ("parallax", "<f4"), ("ncand", "<i4"),
                            ("ngood", "<i4", (8,)), ("cand_parallax", "<f4", (8,)), ("H21", "<f4", (9,)), ("F21", "<f4", (9,))])
# orbs_pair_t / orbs_problem_t / orbs_sim3_info_t (Sim3Solver, sim3_ransac_batch)
SIM3_PAIR_DTYPE = np.dtype([("w1", "<f4", (3,)), ("w2", "<f4", (3,)), ("sigma2_1", "<f4"), ("sigma2_2", "<f4")])
SIM3_PROBLEM_DTYPE = np.dtype([("Tcw1", "<f4", (16,)), ("Tcw2", "<f4", (16,)), ("K1", "<f4", (4,)), ("K2", "<f4", (4,)),
                               ("fix_scale", "<i4"), ("min_inliers", "<i4")])
SIM3_INFO_DTYPE = np.dtype([("n", "<i4"), ("iterations", "<i4"), ("hit_iteration", "<i4"), ("best_iteration", "<i4"),
                            ("best_inliers", "<i4"), ("s", "<f4"), ("R", "<f4", (9,)), ("t", "<f4", (3,)), ("T12", "<f4", (16,))])
# orbz_sim3_match_t / orbz_sim3_problem_t / orbz_sim3_info_t (Optimizer::OptimizeSim3, optimize_sim3*)
SIM3OPT_MATCH_DTYPE = np.dtype([("w1", "<f4", (3,)), ("w2", "<f4", (3,)), ("u1", "<f4"), ("v1", "<f4"), ("u2", "<f4"), ("v2", "<f4"),
                                ("inv_sigma2_1", "<f4"), ("inv_sigma2_2", "<f4")])
SIM3OPT_PROBLEM_DTYPE = np.dtype([("Tcw1", "<f4", (16,)), ("Tcw2", "<f4", (16,)), ("K1", "<f4", (4,)), ("K2", "<f4", (4,)), ("s", "<f4"),
                                  ("R", "<f4", (9,)), ("t", "<f4", (3,)), ("th2", "<f4"), ("fix_scale", "<i4")])
SIM3OPT_INFO_DTYPE = np.dtype([("correspondences", "<i4"), ("bad", "<i4"), ("rounds", "<i4"), ("iterations", "<i4", (2,)),
                               ("trials", "<i4", (2,)), ("reserved", "<i4"), ("q", "<f8", (4,)), ("t", "<f8", (3,)), ("s", "<f8")])
# orbb_keyframe_t / orbb_point_t / orbb_observation_t / orbb_schedule_t / orbb_info_t (Optimizer::LocalBundleAdjustment, local_bundle_adjustment)
LBA_KEYFRAME_DTYPE = np.dtype([("Tcw", "<f4", (16,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("bf", "<f4"), ("fixed", "<i4")])
LBA_POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")])
LBA_OBSERVATION_DTYPE = np.dtype([("kf", "<i4"), ("pt", "<i4"), ("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("inv_sigma2", "<f4")])
LBA_SCHEDULE_DTYPE = np.dtype([("rounds", "<i4"), ("iterations", "<i4", (2,)), ("robust", "<i4", (2,)), ("delta_mono", "<f4"), ("delta_stereo", "<f4"),
                               ("classify", "<i4"), ("check_stop_first", "<i4")])
LBA_INFO_DTYPE = np.dtype([("rounds", "<i4"), ("iterations", "<i4", (2,)), ("trials", "<i4", (2,)), ("free_poses", "<i4", (2,)), ("stopped_at", "<i4"),
                           ("stop_poll", "<i4"), ("polls", "<i4"), ("erased", "<i4")])
# orbb_blocked_info_t: per round the blocks of the reduced system's pattern, the panels of the blocked LDL^T and the contributions summed
# into the blocks; launches: kernel launches of the call
LBA_BLOCKED_INFO_DTYPE = np.dtype([("blocks", "<i4", (2,)), ("panels", "<i4", (2,)), ("contributions", "<i8", (2,)), ("launches", "<i8")])
LBA_STOP_BEFORE, LBA_STOP_ROUND1, LBA_STOP_BETWEEN, LBA_STOP_ROUND2 = 1, 2, 3, 4      # info["stopped_at"]
LBA_MAX_ITERATIONS = 100
# orbg_sim3_t / orbg_vertex_t / orbg_edge_t / orbg_point_t / orbg_info_t (Optimizer::OptimizeEssentialGraph, optimize_essential_graph)
EG_SIM3_DTYPE = np.dtype([("q", "<f8", (4,)), ("t", "<f8", (3,)), ("s", "<f8")])      # q = x y z w
EG_VERTEX_DTYPE = np.dtype([("Scw", EG_SIM3_DTYPE), ("Snc", EG_SIM3_DTYPE), ("has_nc", "<i4"), ("fixed", "<i4")])
EG_EDGE_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("kind", "<i4")])      # kind 0: loop connection, 1: spanning tree / loop / covisibility
EG_POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("ref", "<i4")])
EG_MAX_ITERATIONS = 64
# covisibility (include/orbx.h, orbc_*): the observation table's records
COVIS_KEYFRAME_DTYPE = np.dtype([("id", "<i4"), ("bad", "u1"), ("not_erase", "u1"), ("pad", "u1", (2,)), ("Ow", "<f4", (3,)), ("th_depth", "<f4")])
COVIS_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("ref_kf", "<i4"), ("bad", "u1"), ("pad", "u1", (3,))])
COVIS_OBSERVATION_DTYPE = np.dtype([("kf", "<i4"), ("idx", "<i4"), ("octave", "u1"), ("stereo", "u1"), ("pad", "u1", (2,))])
COVIS_FEATURE_DTYPE = np.dtype([("point", "<i4"), ("octave", "<i4"), ("depth", "<f4")])
COVIS_NORMAL_DTYPE = np.dtype([("normal", "<f4", (3,)), ("max_distance", "<f4"), ("min_distance", "<f4"), ("status", "<i4")])
COVIS_LDS_KEYFRAMES = 8192           # ORBC_LDS_KEYFRAMES: k_cov_count's counters of one query live in LDS up to this K
COVIS_SORT_LDS = 1024                # ORBC_SORT_LDS: k_cov_order sorts a list in LDS up to this length
COVIS_MAX_CULL_KEYFRAMES = 262144    # ORBC_MAX_CULL_KEYFRAMES
# the local map (include/orbx.h, orbt_*): a point's view record and the rule fields of a frame's result
LOCALMAP_VIEW_DTYPE = np.dtype([("normal", "<f4", (3,)), ("max_distance", "<f4"), ("min_distance", "<f4"), ("observations", "<i4")])
LOCALMAP_INFO_DTYPE = np.dtype([("empty_vote", "<i4"), ("n_voted", "<i4"), ("ref_kf", "<i4"), ("ref_votes", "<i4"), ("extension_end", "<i4"),
                                ("launches", "<i4"), ("syncs", "<i4"), ("pad", "<i4")])
LOCALMAP_END_RAN_OUT, LOCALMAP_END_LENGTH, LOCALMAP_END_PARENT = 0, 1, 2      # ORBT_END_*
EG_INFO_DTYPE = np.dtype([("iterations", "<i4"), ("trials", "<i4"), ("end", "<i4"), ("free_vertices", "<i4"), ("blocks", "<i4"), ("levels", "<i4"),
                          ("launches", "<i4"), ("pad", "<i4"), ("chi2_first", "<f8"), ("chi2_last", "<f8"), ("trials_it", "<i4", (EG_MAX_ITERATIONS,))])
EG_END_ITERATIONS, EG_END_QMAX, EG_END_RHO0, EG_END_SOLVER, EG_END_NBAD = 0, 1, 2, 3, 4      # info["end"]
# orbl_view_t / orbl_stereo_t / orbl_point_t (LocalMapping::CreateNewMapPoints, triangulate_new_points*)
NEWPOINT_VIEW_DTYPE = np.dtype([("Tcw", "<f4", (16,)), ("Ow", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"),
                                ("invfx", "<f4"), ("invfy", "<f4"), ("mb", "<f4"), ("mbf", "<f4"), ("scale_factor", "<f4"), ("nlevels", "<i4")])
NEWPOINT_STEREO_DTYPE = np.dtype([("ur", "<f4"), ("depth", "<f4"), ("raw_u", "<f4"), ("raw_v", "<f4")])
NEWPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("status", "<i4"), ("cos_rays", "<f4"), ("cos_stereo", "<f4"),
                           ("reserved", "<i4", (2,))])
NEWPOINT_TRIANGULATED, NEWPOINT_STEREO1, NEWPOINT_STEREO2 = 0, 1, 2      # status >= 0: accepted; the negative ones: include/orbx.h
NEWPOINT_MAX_LEVELS = 16
# orbp_corr_t / orbp_problem_t / orbp_pnp_info_t (PnPsolver, pnp_ransac_batch)
PNP_CORR_DTYPE = np.dtype([("w", "<f4", (3,)), ("u", "<f4"), ("v", "<f4"), ("sigma2", "<f4")])
PNP_PROBLEM_DTYPE = np.dtype([("K", "<f4", (4,)), ("th2", "<f4"), ("min_inliers", "<i4"), ("max_iterations", "<i4"),
                              ("iterations_done", "<i4"), ("prior_best_inliers", "<i4")])
PNP_INFO_DTYPE = np.dtype([("n", "<i4"), ("iterations", "<i4"), ("hit_iteration", "<i4"), ("iterations_run", "<i4"),
                           ("best_iteration", "<i4"), ("best_inliers", "<i4"), ("refined_inliers", "<i4"), ("no_more", "<i4"),
                           ("pose", "<i4"), ("Tcw", "<f4", (16,)), ("best_Tcw", "<f4", (16,))])
PNP_POSE_NONE, PNP_POSE_REFINED, PNP_POSE_BEST, PNP_POSE_PRIOR_BEST = 0, 1, 2, 3
DB_HIT_DTYPE = np.dtype([("kf_id", "<i4"), ("words", "<i4"), ("flags", "<u4"), ("score", "<f4"), ("acc_score", "<f4"), ("best_kf", "<i4")])
DB_MAX_KF_ID, DB_MAX_QUERY, DB_MAX_COVISIBLE = (1 << 20) - 1, 8192, 10

ORBX_OK, ORBX_ERR_ARG, ORBX_ERR_NO_DEVICE, ORBX_ERR_HIP, ORBX_ERR_CAPACITY, ORBX_ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5
NUM_STAGES = 5

# every symbol include/orbx.h declares (tests check the library exports all of them)
EXPORTS = [
    "orbx_create", "orbx_destroy", "orbx_get_levels", "orbx_get_scale_factor", "orbx_get_tables",
    "orbx_max_keypoints", "orbx_extract", "orbx_extract_batch", "orbx_extract_batch_device",
    "orbx_pyramid_host", "orbx_pyramid_device", "orbx_level_counts", "orbx_set_profiling",
    "orbx_get_stage_ms", "orbx_create_flavoured", "orbx_get_flavour", "orbx_set_option", "orbx_get_option", "orbm_set_thread_option", "orbm_hamming", "orbm_hamming_matrix_device", "orbm_stereo_batch_device",
    "orbm_stereo", "orbm_search_for_initialization", "orbm_search_by_projection_mp",
    "orbm_search_by_projection_frame", "orbm_match_windows", "orbm_best_in_windows", "orbm_distinctive_descriptors", "orbm_predict_scale_thresholds", "orbm_is_in_frustum",
    "orbm_search_local_points", "orbv_create", "orbv_load_text", "orbv_destroy", "orbv_info", "orbv_transform",
    "orbm_search_by_bow", "orbm_search_for_triangulation", "orbx_last_error", "orbx_version", "orbx_device_count",
    "orbx_record_bytes", "orbx_pack_records_device", "orbx_thread_release_scratch",
    "orbm_search_by_projection_frame_device", "orbm_search_local_points_device", "orbx_fast_kernels", "orbx_extract_batch_device_prefetch", "orbx_stream_wait_fast_stage", "orbx_side_stream", "orbm_stereo_batch_device_prev",
    "orbx_side_stream_for", "orbx_stereo_frame", "orbx_set_pyramid_buffers",
    "orbx_stereo_frame_view", "orbx_host_alloc", "orbx_host_free",
    "orbx_gray_from_color_device", "orbm_rgbd_batch_device", "orbx_rgbd_frame",
    "orbx_rectifier_create", "orbx_rectifier_destroy", "orbx_rectifier_maps", "orbx_rectifier_info", "orbx_rectify_device",
    "orbx_stereo_frame_rectified", "orbx_stereo_frame_view_rectified",
    "orbx_cloudmapper_create", "orbx_cloudmapper_destroy", "orbx_cloud_capacity", "orbx_cloud_generate_device",
    "orbx_cloud_voxel_device", "orbx_keyframe_cloud",
    "orbx_octree_device", "orbx_octomap_bt", "orbx_octomap_bytes_bound",
    "orbv_score_l1", "orbv_db_create", "orbv_db_destroy", "orbv_db_add", "orbv_db_erase", "orbv_db_clear", "orbv_db_set_covisible",
    "orbv_db_info", "orbv_db_score", "orbv_db_detect_loop", "orbv_db_detect_reloc",
    "orbx_level0_layout", "orbx_extract_batch_device_padded", "orbx_extract_batch_device_padded_prefetch",
]
# the optimiser section of include/orbx.h (prefix orbo_), listed apart: EXPORTS is compared with the header's orbx_ / orbm_ / orbv_ names
POSE_EXPORTS = ["orbo_pose_optimization", "orbo_pose_optimization_batch", "orbo_pose_optimization_device"]
# the initialiser section (prefix orbi_), apart for the same reason
INIT_EXPORTS = ["orbi_initialize", "orbi_initialize_device", "orbi_search"]
# the Sim3Solver section (prefix orbs_), apart for the same reason
SIM3_EXPORTS = ["orbs_sim3_iterations", "orbs_sim3_ransac", "orbs_sim3_ransac_batch"]
# the PnPsolver section (prefix orbp_), apart for the same reason
PNP_EXPORTS = ["orbp_pnp_parameters", "orbp_pnp_ransac", "orbp_pnp_ransac_batch"]
# the Sim3 optimiser section (prefix orbz_; orbo_ is PoseOptimization's), apart for the same reason
SIM3OPT_EXPORTS = ["orbz_optimize_sim3", "orbz_optimize_sim3_batch"]
# the LocalMapping section (prefix orbl_), apart for the same reason
NEWPOINTS_EXPORTS = ["orbl_triangulate", "orbl_triangulate_batch", "orbl_baseline_ok", "orbl_compute_f12", "orbl_create_new_map_points"]
# the bundle adjustment section (prefix orbb_), apart for the same reason
LBA_EXPORTS = ["orbb_optimize", "orbb_local_bundle_adjustment", "orbb_bundle_adjustment", "orbb_optimize_blocked", "orbb_global_bundle_adjustment"]
# the essential graph section (prefix orbg_), apart for the same reason
ESSENTIAL_EXPORTS = ["orbg_optimize_essential_graph"]
COVIS_EXPORTS = ["orbc_covisibility", "orbc_update_connections", "orbc_keyframe_culling", "orbc_update_normal_and_depth"]
# the local map section (prefix orbt_), apart for the same reason
LOCALMAP_EXPORTS = ["orbt_localmap_create", "orbt_localmap_destroy", "orbt_localmap_info", "orbt_localmap_set_map", "orbt_update_local_map"]
# loop map correction (prefix orbr_), apart for the same reason
MAPCORRECT_EXPORTS = ["orbr_correct_loop", "orbr_spread_global_ba"]
MAPCORRECT_NORMAL_UNTOUCHED = 4      # ORBR_NORMAL_UNTOUCHED: no query owns the point (the other codes of a normal's status are ORBC_NORMAL_*)
MAPCORRECT_SPREAD_UNTOUCHED, MAPCORRECT_SPREAD_GBA, MAPCORRECT_SPREAD_MOVED, MAPCORRECT_SPREAD_UNDEFINED = 0, 1, 2, 3      # ORBR_SPREAD_*
# what include/orbx_dev.h declares on top: exported by the developer build only
DEV_EXPORTS = ["orbx_debug_level_points", "orbx_debug_sincosf", "orbx_debug_blur_patches", "orbm_debug_features_in_area",
               "orbx_debug_blurred_level", "orbx_debug_octree_fallbacks", "orbm_debug_match_path", "orbm_debug_resolve_plan",
               "orbm_debug_stereo_path", "orbx_debug_plan_chunk", "orbx_debug_last_plan", "orbm_debug_thread_scratch",
               "orbx_debug_size_plan", "orbx_debug_set_alloc_fill", "orbx_debug_alloc_fill_stats", "orbx_debug_stall_stream",
               "orbx_debug_streams"]
# what include/orbx_dev_pyr.h declares: the developer build's hook for k_pyr_level's records (debug_pyr_records)
DEV_PYR_EXPORTS = ["orbx_debug_pyr_records"]
# what include/orbx_dev_level0.h declares: which input form the last extraction call ran (ORBextractor.level0_in_place)
DEV_LEVEL0_EXPORTS = ["orbx_debug_level0_in_place"]
# include/orbx_dev.h: the int64 record of orbx_debug_size_plan, field order
SIZE_PLAN_FIELDS = ["max_kp", "totalCells", "maxNodeCap", "lvlKpCap", "pyrImgBytes", "slotsPerImg", "keysPerImg", "fastTileStride", "fastScoreStride",
                    "fastTileRows", "fastLdsPerWave", "totalStrips", "stripLevels", "octLdsBytes", "octPyrLdsBytes", "octPyrWords", "octBigMask",
                    "octDeepMax", "octSliceStride", "histStride", "pyrTilesX", "pyrTilesY", "pyrXSpanOff", "pyrYSpanOff", "pyrBufBytes", "pyrMaxDim",
                    "pyrMaxPar", "pyrLdsBytes", "nChains0", "nChains1", "tabWords"]   # + stripBase[17] + chains[2][8][8]
# csrc/orbx_size_plan.h: LevelGeom as the kernels read it (144 bytes)
LEVEL_GEOM_DTYPE = np.dtype([("w", "<i4"), ("h", "<i4"), ("pstride", "<i4"), ("prows", "<i4"), ("poff", "<u8"), ("regW", "<i4"), ("regH", "<i4"),
                             ("nCols", "<i4"), ("nRows", "<i4"), ("wCell", "<i4"), ("hCell", "<i4"), ("cellBase", "<i4"), ("ncells", "<i4"),
                             ("capc", "<i4"), ("pad_", "<i4"), ("slotOff", "<u8"), ("N", "<i4"), ("nIni", "<i4"), ("nodeCap", "<i4"),
                             ("pyrDepth", "<i4"), ("keyOff", "<u8"), ("keyCap", "<i4"), ("lvlKpOff", "<i4"), ("xofsOff", "<i4"), ("xalphaOff", "<i4"),
                             ("yofsOff", "<i4"), ("ybetaOff", "<i4"), ("rootTabOff", "<i4"), ("rootBoxOff", "<i4"), ("xPathOff", "<i4"),
                             ("yPathOff", "<i4"), ("scale", "<f4"), ("size", "<f4")])
# include/orbx_dev.h: the record orbm_debug_thread_scratch fills, field order
THREAD_SCRATCH_FIELDS = ["arena_cap", "arena_device", "arena_seq", "arena_stream", "arena_word", "stage_cap", "stage_device", "bow_cap",
                         "bow_device"]
# include/orbx_dev.h: PlanInput / ChunkPlan of the launch rule as flat int32 arrays (orbx_debug_plan_chunk, orbx_debug_last_plan), field order
PLAN_INPUT_FIELDS = ["B", "nl", "totalStrips", "stripLevels", "octBigMask", "lastChunks", "prof", "profFast", "skipPyr", "pfUsed", "evPyrDone",
                     "dbgBlur", "sliceScratch", "fastTileStride", "fastScoreStride", "sparseRecent"]   # + ncells[16] + opt[32]
CHUNK_PLAN_FIELDS = ["usePyr", "strips", "stripLevels", "fastCells", "es", "histOct", "multiWg", "fused", "gather", "bigMask", "wideOct", "compact",
                     "sparseForm", "sparsePerCell", "rowFlags", "sparseHint", "earlyLv", "aSplit", "octForm", "sweepSlices", "sweepShared",
                     "orderKernel", "fastDoneAt", "fastPhase", "octPhase", "octStop", "descLdsPad"]   # + nslice[16]
OCT_EXACT, OCT_BIG, OCT_EARLY, OCT_SPLIT, OCT_SINGLE = 0, 1, 2, 3, 4      # ChunkPlan.octForm
HINT_NONE, HINT_OCT_SRC, HINT_GATHER = 0, 1, 2                            # ChunkPlan.sparseHint
# include/orbx_dev.h: ORBM_PATH_RES_* / ORBM_PATH_FB_* (orbm_debug_match_path, orbm_debug_resolve_plan)
RES_NONE, RES_PAR_Q2, RES_PAR_Q4, RES_WAVE, RES_EXACT = 0, 1, 2, 3, 4
FB_NONE, FB_N, FB_INIT_SIZE, FB_CAND_CAP, FB_QK, FB_LDS, FB_OPTION = 0, 1, 2, 3, 4, 5, 6


class OrbxError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("orbx status %d: %s" % (status, msg))
        self.status = status


class StereoView(C.Structure):
    """orbx_stereo_view_t (orbx_stereo_frame_view)."""
    _fields_ = [("nl", C.c_int32), ("nr", C.c_int32), ("nmatch", C.c_int32), ("cap", C.c_int32),
                ("kl", C.c_void_p), ("kr", C.c_void_p), ("dl", C.c_void_p), ("dr", C.c_void_p), ("uright", C.c_void_p), ("depth", C.c_void_p),
                ("d_kl", C.c_void_p), ("d_kr", C.c_void_p), ("d_dl", C.c_void_p), ("d_dr", C.c_void_p), ("d_uright", C.c_void_p),
                ("d_depth", C.c_void_p)]


class OctreeInfo(C.Structure):
    """orbx_octree_info_t (orbx_octree_device / orbx_octomap_bt)."""
    _fields_ = [("points_in", C.c_int64), ("points_dropped", C.c_int64), ("cells", C.c_int64), ("leaves", C.c_int64),
                ("tree_size", C.c_int64), ("data_bytes", C.c_int64), ("overflow", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        return {f: int(getattr(self, f)) for f, _ in self._fields_ if f != "reserved"}


class Level0Layout(C.Structure):
    """orbx_level0_layout_t: the layout of in-place input (orbx_level0_layout / orbx_extract_batch_device_padded)."""
    _fields_ = [("pstride", C.c_int32), ("prows", C.c_int32), ("pixel0_offset", C.c_uint64), ("image_bytes", C.c_uint64)]


def level0_layout(w, h, nlevels=8, scale_factor=1.2, developer=False):
    """No HIP call (works without a GPU): where a caller of ORBextractor.extract_batch_device_padded puts a w x h frame -> dict(pstride,
    prows, pixel0_offset, image_bytes); raises OrbxError for a size an extractor with these levels refuses."""
    L = lib(developer)
    out = Level0Layout()
    _check(L.orbx_level0_layout(int(w), int(h), int(nlevels), float(scale_factor), C.byref(out)), L)
    return {f: int(getattr(out, f)) for f, _ in out._fields_}


class GridGeom(C.Structure):
    """orbm_grid_geom_t (src/Frame.cc:90-105)."""
    _fields_ = [("min_x", C.c_float), ("min_y", C.c_float), ("max_x", C.c_float), ("max_y", C.c_float),
                ("inv_w", C.c_float), ("inv_h", C.c_float)]


class Camera(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("mbf", C.c_float), ("mb", C.c_float)]


class RGBDCamera(C.Structure):
    """orbx_rgbd_camera_t: mK, mDistCoef (k1 k2 p1 p2 k3; k3 = 0 for a 4-element mDistCoef) and mbf of an RGB-D Frame."""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("k1", C.c_float), ("k2", C.c_float),
                ("p1", C.c_float), ("p2", C.c_float), ("k3", C.c_float), ("mbf", C.c_float)]


# depth image element types of orbx_rgbd_frame / orbm_rgbd_batch_device (OpenCV's CV_16U / CV_32F)
DEPTH_U16, DEPTH_F32 = 2, 5
_DEPTH_TYPES = {np.dtype(np.uint16): DEPTH_U16, np.dtype(np.float32): DEPTH_F32}


def grid_geom(w, h):
    """Grid of an undistorted camera: mnMinX=0, mnMaxX=cols (src/Frame.cc:469-478)."""
    g = GridGeom()
    g.min_x, g.min_y, g.max_x, g.max_y = 0.0, 0.0, float(w), float(h)
    g.inv_w = np.float32(64) / np.float32(w)
    g.inv_h = np.float32(48) / np.float32(h)
    return g


class Flavour(C.Structure):
    """orbx_flavour_t: which OpenCV build the handle stands in for (include/orbx.h)."""
    _fields_ = [("gauss_rounding", C.c_int32), ("gauss_taps", C.c_int32 * 4), ("reserved", C.c_int32 * 3)]


GAUSS_FLAVOURS = {"half_up": 0, "sse2": 1}
GAUSS_FIXED_TAPS = 2


def parse_gauss(g):
    """"half_up" | "sse2" | "taps:k0,k1,k2,k3" (ORBX_GAUSS_FIXED_TAPS: the build's Q8 taps, centre first) -> Flavour."""
    fl = Flavour()
    if isinstance(g, str) and g.startswith("taps:"):
        taps = [int(v) for v in g[5:].split(",")]
        if len(taps) != 4:
            raise ValueError("bad gauss flavour %r (taps:k0,k1,k2,k3)" % (g,))
        fl.gauss_rounding = GAUSS_FIXED_TAPS
        for i, v in enumerate(taps):
            fl.gauss_taps[i] = v
    elif g in GAUSS_FLAVOURS:
        fl.gauss_rounding = GAUSS_FLAVOURS[g]
    else:
        raise ValueError("bad gauss flavour %r" % (g,))
    return fl
# What an ORBextractor takes when its constructor is not told.  HARNESS state of this Python module (the library itself has no
# process-global switch: flavour and options are per handle): the parity suite is run under both flavours by changing this and the
# oracle's default together, and the tests that cover an alternative kernel set a default option around the code under test.
# ORBX_TEST_GAUSS_FLAVOUR=sse2 in the environment runs a whole test / bench session (spawned oracle workers included) under the
# other flavour.
default_gauss_flavour = os.environ.get("ORBX_TEST_GAUSS_FLAVOUR", "half_up")
_default_options = {}
_live = None


def set_default_option(key, value):
    """Option `key` of every ORBextractor created from now on AND of the live ones (value 0 = the library default)."""
    if value:
        _default_options[int(key)] = int(value)
    else:
        _default_options.pop(int(key), None)
    for e in list(_live or ()):
        if getattr(e, "_h", None):
            e.set_option(key, value)


_lib = None
_dev_lib = None


def build(force=False):
    from . import build as _b
    return _b.build(force=force)


def _preload_shared_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so and
    request it by the un-versioned name, so if our library pulled in /opt/rocm's copy first, a
    later `import torch` would start a SECOND runtime (whose device init then fails and whose
    pointers/streams are foreign to ours).  When torch is installed, load its copy first; our
    library's NEEDED libamdhip64.so.7 then binds to it by soname, whatever the import order."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec and spec.submodule_search_locations:
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            try:
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
            except OSError:
                pass


def lib(developer=False):
    """Load the HIP library (developer = True: the developer build with the stage hooks); fails loudly when it has not been built."""
    global _lib, _dev_lib
    if developer:
        if _dev_lib is None:
            _dev_lib = _load(DEV_LIB_PATH, True)
        return _dev_lib
    if _lib is None:
        _lib = _load(LIB_PATH, os.path.basename(LIB_PATH) == "liborbx_hip_dev.so")
    return _lib


LBA_STOP_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)      # int (*stop)(void *): pbStopFlag of Optimizer::LocalBundleAdjustment


def matcher_lib():
    """The library the matcher functions of this module call: the developer build while default_developer is True (`hooks` fixture),
    so that the path hooks below and orbm_set_thread_option act on the library that ran the call (both are per library)."""
    return lib(default_developer)


def _load(path, dev):
    if not os.path.exists(path):
        raise OrbxError(ORBX_ERR_NO_DEVICE, "HIP library %s is missing: run `python __graft_entry__.py` "
                                            "(build()) first; there is no CPU fallback" % path)
    _preload_shared_hip_runtime()
    L = C.CDLL(path)
    vp, i32, f32, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    L.orbx_create.restype = i32
    L.orbx_create.argtypes = [i32, f32, i32, i32, i32, i32, C.POINTER(vp)]
    L.orbx_destroy.argtypes = [vp]
    L.orbx_create_flavoured.argtypes = [i32, f32, i32, i32, i32, i32, C.POINTER(Flavour), C.POINTER(vp)]
    L.orbx_get_flavour.argtypes = [vp, C.POINTER(Flavour)]
    L.orbx_set_option.argtypes = [vp, i32, i32]
    L.orbx_get_option.argtypes = [vp, i32, C.POINTER(i32)]
    L.orbm_set_thread_option.argtypes = [i32, i32]
    L.orbx_get_levels.argtypes = [vp]
    L.orbx_get_scale_factor.restype = f32
    L.orbx_get_scale_factor.argtypes = [vp]
    L.orbx_get_tables.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.orbx_max_keypoints.argtypes = [vp]
    L.orbx_extract.argtypes = [vp, vp, i32, i32, i32, vp, vp, i32, C.POINTER(i32)]
    L.orbx_extract_batch.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, i32, vp]
    L.orbx_extract_batch_device.argtypes = [vp, vp, i32, i32, i32, i32, sz, vp, vp, vp, i32, vp]
    L.orbx_extract_batch_device_prefetch.argtypes = [vp, vp, i32, i32, i32, i32, sz, vp]
    L.orbx_extract_batch_device_padded.argtypes = [vp, vp, i32, i32, i32, sz, vp, vp, vp, i32, vp]
    L.orbx_extract_batch_device_padded_prefetch.argtypes = [vp, vp, i32, i32, i32, sz, vp]
    L.orbx_level0_layout.argtypes = [i32, i32, i32, f32, C.POINTER(Level0Layout)]
    L.orbx_stream_wait_fast_stage.argtypes = [vp, vp]
    L.orbx_side_stream.argtypes = [vp]
    L.orbx_side_stream.restype = vp
    L.orbx_stereo_frame.argtypes = [vp, vp, vp, i32, i32, i32, f32, f32, i32, vp, vp, C.POINTER(i32), vp, vp, C.POINTER(i32), vp, vp,
                                    C.POINTER(i32)]
    L.orbx_stereo_frame_view.argtypes = [vp, vp, vp, i32, i32, i32, f32, f32, vp]
    L.orbx_gray_from_color_device.argtypes = [vp, i32, i32, i32, i32, i32, i32, sz, vp, i32, sz, vp]
    L.orbm_rgbd_batch_device.argtypes = [vp, vp, i32, i32, vp, i32, i32, i32, i32, sz, f32, C.POINTER(RGBDCamera), vp, vp, vp, vp]
    L.orbx_rgbd_frame.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, i32, i32, f32, C.POINTER(RGBDCamera), i32, vp, vp,
                                  C.POINTER(i32), vp, vp, vp]
    L.orbx_rectifier_create.argtypes = [vp, vp, i32, vp, vp, i32, i32, i32, C.POINTER(vp)]
    L.orbx_rectifier_destroy.argtypes = [vp]
    L.orbx_rectifier_maps.argtypes = [vp, vp, vp]
    L.orbx_rectifier_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(sz)]
    L.orbx_rectify_device.argtypes = [vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, sz, vp, i32, sz, vp]
    L.orbx_stereo_frame_rectified.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, f32, i32, vp, vp, C.POINTER(i32), vp, vp,
                                              C.POINTER(i32), vp, vp, C.POINTER(i32)]
    L.orbx_stereo_frame_view_rectified.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, f32, vp]
    L.orbx_cloudmapper_create.argtypes = [f32, i32, i32, i32, C.POINTER(vp)]
    L.orbx_cloudmapper_destroy.argtypes = [vp]
    L.orbx_cloud_capacity.argtypes = [i32, i32, i32]
    L.orbx_cloud_generate_device.argtypes = [vp, vp, i32, i32, sz, f32, vp, i32, i32, sz, i32, i32, i32, f32, f32, f32, f32, vp, vp, i32, vp, vp]
    L.orbx_cloud_voxel_device.argtypes = [vp, vp, vp, i32, i32, vp, i32, vp, vp]
    L.orbx_keyframe_cloud.argtypes = [vp, vp, i32, i32, vp, i32, i32, f32, i32, i32, f32, f32, f32, f32, vp, i32, vp, C.POINTER(i32), vp,
                                      C.POINTER(i32)]
    L.orbx_octree_device.argtypes = [vp, vp, vp, i32, i32, vp, C.c_double, vp, C.c_int64, vp, C.c_int64, vp, vp]
    L.orbx_octomap_bt.argtypes = [vp, vp, i32, vp, C.c_double, vp, sz, C.POINTER(sz), C.POINTER(OctreeInfo)]
    L.orbx_octomap_bytes_bound.argtypes = [C.c_int64]
    L.orbx_octomap_bytes_bound.restype = sz
    L.orbx_host_alloc.argtypes = [sz]
    L.orbx_host_alloc.restype = vp
    L.orbx_host_free.argtypes = [vp]
    L.orbx_host_free.restype = None
    L.orbx_set_pyramid_buffers.argtypes = [vp, i32]
    L.orbx_side_stream_for.argtypes = [vp, vp]
    L.orbx_side_stream_for.restype = vp
    L.orbx_pyramid_host.argtypes = [vp, i32, i32, i32, vp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.orbx_pyramid_device.argtypes = [vp, i32, i32, C.POINTER(vp), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.orbx_level_counts.argtypes = [vp, i32, vp, vp]
    L.orbx_set_profiling.argtypes = [vp, i32]
    L.orbx_fast_kernels.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.orbx_record_bytes.argtypes = [i32]
    L.orbx_pack_records_device.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp, vp]
    L.orbx_get_stage_ms.argtypes = [vp, vp, C.POINTER(i32)]
    L.orbm_hamming.argtypes = [vp, vp]
    L.orbm_hamming_matrix_device.argtypes = [vp, i32, vp, i32, vp, vp]
    L.orbm_stereo_batch_device.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, f32, f32, vp, vp, vp, vp]
    L.orbm_stereo_batch_device_prev.argtypes = L.orbm_stereo_batch_device.argtypes
    L.orbm_stereo.argtypes = [vp, vp, vp, vp, i32, vp, vp, i32, f32, f32, vp, vp, C.POINTER(i32)]
    L.orbm_search_for_initialization.argtypes = [vp, vp, i32, vp, vp, i32, C.POINTER(GridGeom), vp, vp, i32, f32,
                                                 i32, i32, C.POINTER(i32)]
    L.orbm_search_by_projection_mp.argtypes = [vp, vp, vp, i32, C.POINTER(GridGeom), vp, i32, vp, vp, i32, vp, vp,
                                               f32, f32, i32, C.POINTER(i32)]
    L.orbm_search_by_projection_frame.argtypes = [vp, vp, vp, i32, C.POINTER(GridGeom), vp, i32, C.POINTER(Camera),
                                                  vp, vp, vp, vp, i32, vp, vp, f32, i32, i32, i32, C.POINTER(i32)]
    L.orbm_search_by_projection_frame_device.argtypes = L.orbm_search_by_projection_frame.argtypes + [vp]
    L.orbm_match_windows.argtypes = [vp, vp, vp, i32, C.POINTER(GridGeom), C.POINTER(GridGeom), vp, vp, i32, vp, vp, i32, i32, i32, C.POINTER(i32)]
    L.orbm_distinctive_descriptors.argtypes = [vp, vp, i32, vp, vp, i32]
    L.orbm_predict_scale_thresholds.argtypes = [f32, i32, vp]
    L.orbv_create.argtypes = [i32, i32, i32, i32, i32, vp, vp, vp, vp, i32, C.POINTER(vp)]
    L.orbv_load_text.argtypes = [C.c_char_p, i32, C.POINTER(vp)]
    L.orbv_destroy.argtypes = [vp]
    L.orbv_destroy.restype = None
    L.orbv_info.argtypes = [vp] + [C.POINTER(i32)] * 6
    L.orbv_transform.argtypes = [vp, vp, i32, i32, vp, vp, vp]
    L.orbv_score_l1.argtypes = [vp, vp, i32, vp, vp, i32, vp]
    L.orbv_db_create.argtypes = [i32, i32, i32, C.POINTER(vp)]
    L.orbv_db_destroy.argtypes = [vp]
    L.orbv_db_destroy.restype = None
    L.orbv_db_add.argtypes = [vp, i32, vp, vp, i32]
    L.orbv_db_erase.argtypes = [vp, i32]
    L.orbv_db_clear.argtypes = [vp]
    L.orbv_db_set_covisible.argtypes = [vp, i32, vp, i32]
    L.orbv_db_info.argtypes = [vp, C.POINTER(i32), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(sz)]
    L.orbv_db_score.argtypes = [vp, vp, vp, i32, vp, i32, vp]
    L.orbv_db_detect_loop.argtypes = [vp, vp, vp, i32, vp, i32, f32, vp, i32, C.POINTER(i32), vp, i32, C.POINTER(i32)]
    L.orbv_db_detect_reloc.argtypes = [vp, vp, vp, i32, vp, i32, C.POINTER(i32), vp, i32, C.POINTER(i32)]
    L.orbm_search_for_triangulation.argtypes = [vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, i32, vp, f32, f32, vp, vp, i32, i32, i32, vp,
                                                C.POINTER(i32), i32]
    L.orbm_search_by_bow.argtypes = [vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, i32, i32, f32, i32, vp, C.POINTER(i32), i32]
    L.orbm_is_in_frustum.argtypes = [vp, i32, vp, C.POINTER(Camera), C.POINTER(GridGeom), f32, vp, i32, vp, i32]
    L.orbm_search_local_points.argtypes = [vp, vp, vp, i32, C.POINTER(GridGeom), vp, i32, vp, vp, i32, vp, C.POINTER(Camera), f32,
                                           vp, vp, vp, f32, f32, i32, C.POINTER(i32), vp]
    L.orbm_search_local_points_device.argtypes = L.orbm_search_local_points.argtypes + [vp]
    L.orbo_pose_optimization.argtypes = [vp, i32, C.POINTER(Camera), vp, vp, vp, C.POINTER(i32), vp, i32]
    L.orbo_pose_optimization_batch.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, i32]
    L.orbo_pose_optimization_device.argtypes = [vp, vp, i32, vp, i32, vp, C.POINTER(Camera), vp, vp, vp, C.POINTER(i32), vp, i32, vp]
    L.orbm_best_in_windows.argtypes = [vp, vp, vp, i32, C.POINTER(GridGeom), C.POINTER(GridGeom), vp, vp, i32, vp, i32, vp, vp, i32]
    L.orbi_initialize.argtypes = [vp, i32, vp, i32, vp, i32, vp, i32, vp, f32, f32, i32, C.POINTER(i32), vp, vp, vp, vp, vp, i32]
    L.orbi_initialize_device.argtypes = L.orbi_initialize.argtypes + [vp]
    L.orbi_search.argtypes = [vp, i32, vp, i32, vp, i32, vp, i32, f32, vp, vp, vp, vp, i32]
    L.orbs_sim3_iterations.argtypes = [i32, C.c_double, i32, i32]
    L.orbs_sim3_ransac.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, i32]
    L.orbs_sim3_ransac_batch.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32]
    L.orbz_optimize_sim3.argtypes = [vp, i32, vp, vp, vp, C.POINTER(i32), vp, i32]
    L.orbz_optimize_sim3_batch.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, i32]
    L.orbl_triangulate.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, vp, C.POINTER(i32), i32]
    L.orbl_triangulate_batch.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32]
    L.orbl_baseline_ok.argtypes = [vp, vp, i32, f32]
    L.orbl_compute_f12.argtypes = [vp, vp, vp, vp, vp]
    L.orbl_create_new_map_points.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32]
    L.orbb_optimize.argtypes = [vp, i32, vp, i32, vp, i32, vp, LBA_STOP_FN, vp, vp, vp, vp, vp, vp, vp, i32]
    L.orbb_local_bundle_adjustment.argtypes = [vp, i32, vp, i32, vp, i32, LBA_STOP_FN, vp, vp, vp, vp, vp, vp, vp, i32]
    L.orbb_bundle_adjustment.argtypes = [vp, i32, vp, i32, vp, i32, i32, i32, LBA_STOP_FN, vp, vp, vp, vp, vp, vp, i32]
    L.orbb_optimize_blocked.argtypes = [vp, i32, vp, i32, vp, i32, vp, LBA_STOP_FN, vp, vp, vp, vp, vp, vp, vp, vp, i32]
    L.orbb_global_bundle_adjustment.argtypes = [vp, i32, vp, i32, vp, i32, i32, i32, LBA_STOP_FN, vp, vp, vp, vp, vp, vp, vp, i32]
    L.orbg_optimize_essential_graph.argtypes = [vp, i32, vp, i32, vp, i32, i32, i32, vp, vp, vp, vp, i32]
    L.orbp_pnp_parameters.argtypes = [i32, C.c_double, i32, i32, i32, f32, C.POINTER(i32), C.POINTER(i32)]
    L.orbp_pnp_ransac.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32]
    L.orbp_pnp_ransac_batch.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32]
    L.orbc_covisibility.argtypes = [vp, vp, vp, vp, vp, vp, i32]
    L.orbc_update_connections.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, i32]
    L.orbc_keyframe_culling.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, i32]
    L.orbc_update_normal_and_depth.argtypes = [vp, vp, i32]
    L.orbt_localmap_create.argtypes = [i32, C.POINTER(vp)]
    L.orbt_localmap_destroy.argtypes = [vp]
    L.orbt_localmap_destroy.restype = None
    L.orbt_localmap_info.argtypes = [vp, vp, vp, vp, vp, vp]
    L.orbt_localmap_set_map.argtypes = [vp, vp]
    L.orbt_update_local_map.argtypes = [vp, vp, i32, vp, i32, i32, i32, vp]
    L.orbr_correct_loop.argtypes = [vp, vp, i32, vp, vp, vp, i32]
    L.orbr_spread_global_ba.argtypes = [vp, vp, i32]
    if dev:
        L.orbx_debug_level_points.argtypes = [vp, i32, i32, i32, vp, i32, C.POINTER(i32)]
        L.orbx_debug_sincosf.argtypes = [vp, i32, vp, vp, i32]
        L.orbx_debug_blur_patches.argtypes = [vp, i32, vp, i32]
        L.orbx_debug_octree_fallbacks.argtypes = [vp, vp, i32]
        L.orbx_debug_blurred_level.argtypes = [vp, i32, i32, vp, i32, vp]
        L.orbm_debug_features_in_area.argtypes = [vp, i32, C.POINTER(GridGeom), f32, f32, f32, i32, i32, vp, C.POINTER(i32), i32]
        L.orbm_debug_match_path.argtypes = [vp]
        L.orbm_debug_resolve_plan.argtypes = [i32, i32, i32, i32, vp]
        L.orbm_debug_stereo_path.argtypes = [vp]
        L.orbx_debug_plan_chunk.argtypes = [vp, i32, vp, i32]
        L.orbx_debug_last_plan.argtypes = [vp, vp, i32]
        L.orbm_debug_thread_scratch.argtypes = [vp, i32]
        L.orbx_debug_size_plan.argtypes = [i32, f32, i32, i32, i32, i32, vp, vp, vp, i32, vp, i32, vp, i32]
        L.orbx_debug_pyr_records.argtypes = [vp, i32, f32, i32, i32, i32, vp, i32, vp, i32, vp, i32]
        L.orbx_debug_level0_in_place.argtypes = [vp]
        L.orbx_debug_set_alloc_fill.argtypes = [i32, C.c_uint32]
        L.orbx_debug_alloc_fill_stats.argtypes = [vp]
        L.orbx_debug_stall_stream.argtypes = [vp, i32, i32]
        L.orbx_debug_streams.argtypes = [vp, vp, i32]
    L.orbx_last_error.restype = C.c_char_p
    L.orbx_version.restype = C.c_char_p
    L._orbx_developer = bool(dev)
    return L


def _check(rc, L=None):
    if rc != 0:
        raise OrbxError(rc, (L or matcher_lib()).orbx_last_error().decode())


def _p(a):
    return a.ctypes.data if a is not None else None      # (an int: every pointer parameter is declared c_void_p; data_as() costs a microsecond more)


def blur_reach_mask():
    """[37, 37] bool: the pixels of a keypoint's blurred block a descriptor tap can reach - the rounded rotation of a pattern point
    with x^2 + y^2 <= 338 satisfies (|row| - 1/2)^2 + (|col| - 1/2)^2 <= 338 (+ 2 of slack), 1133 of 1369 pixels.  The fused blur of
    the descriptor kernel computes nothing else, and ORBextractor.debug_blur_patches reports the rest as 0."""
    d = np.abs(np.arange(-18, 19))
    t = np.where(d > 0, 2 * d - 1, 0)
    return (t[:, None] ** 2 + t[None, :] ** 2) <= 4 * 340


def device_count():
    return lib().orbx_device_count()


class ORBextractor:
    """Mirror of ORB_SLAM2::ORBextractor (reference: include/ORBextractor.h:45-111).

    ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST); calling the object
    on an 8-bit gray image returns (keypoints[KP_DTYPE], descriptors[N,32] uint8); the mask
    argument of the reference is ignored there (src/ORBextractor.cc:1043) and absent here.
    """

    def __init__(self, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device=0, gauss=None, developer=None):
        """gauss: "half_up" / "sse2" / "taps:k0,k1,k2,k3" = orbx_flavour_t (include/orbx.h); None = default_gauss_flavour.
        developer: True = this handle lives in the developer build of the library (stage hooks debug_*); None = default_developer."""
        global _live
        self._L = lib(default_developer if developer is None else developer)
        h = C.c_void_p()
        self.gauss = default_gauss_flavour if gauss is None else gauss
        fl = parse_gauss(self.gauss)
        self._ck(self._L.orbx_create_flavoured(int(nfeatures), float(scaleFactor), int(nlevels), int(iniThFAST),
                                             int(minThFAST), int(device), C.byref(fl), C.byref(h)))
        self._h = h
        self.nfeatures, self.nlevels, self.device = int(nfeatures), int(nlevels), int(device)
        self._shape = None
        if _live is None:
            import weakref
            _live = weakref.WeakSet()
        _live.add(self)
        for k, v in _default_options.items():
            self.set_option(k, v)

    def _ck(self, rc):
        _check(rc, self._L)

    def _hooks(self):
        if not self._L._orbx_developer:
            raise OrbxError(ORBX_ERR_ARG, "stage hooks (debug_*) exist in the developer build only: ORBextractor(..., developer=True)")

    def level_counts(self, b=0):
        """(FAST candidates per level, keypoints kept per level) of image slot b of the last call (orbx_level_counts)."""
        c, k = np.zeros(self.nlevels, np.int32), np.zeros(self.nlevels, np.int32)
        self._ck(self._L.orbx_level_counts(self._h, int(b), _p(c), _p(k)))
        return c, k

    def set_option(self, key, value):
        """orbx_set_option: per-handle choice among kernels / arrangements with identical results (ORBX_OPT_* of include/orbx.h)."""
        self._ck(self._L.orbx_set_option(self._h, int(key), int(value)))

    def get_option(self, key):
        v = C.c_int(0)
        self._ck(self._L.orbx_get_option(self._h, int(key), C.byref(v)))
        return v.value

    def flavour(self):
        fl = Flavour()
        self._ck(self._L.orbx_get_flavour(self._h, C.byref(fl)))
        if fl.gauss_rounding == GAUSS_FIXED_TAPS:
            return "taps:" + ",".join(str(int(v)) for v in fl.gauss_taps)
        return {v: k for k, v in GAUSS_FLAVOURS.items()}[fl.gauss_rounding]

    def close(self):
        if getattr(self, "_h", None):
            self._L.orbx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- getters (include/ORBextractor.h:62-83)
    def GetLevels(self):
        return self._L.orbx_get_levels(self._h)

    def GetScaleFactor(self):
        return self._L.orbx_get_scale_factor(self._h)

    def _tables(self):
        n = self.nlevels
        t = [np.zeros(n, np.float32) for _ in range(4)] + [np.zeros(n, np.int32), np.zeros(16, np.int32)]
        self._ck(self._L.orbx_get_tables(self._h, *[_p(a) for a in t]))
        return t

    def GetScaleFactors(self): return self._tables()[0]
    def GetInverseScaleFactors(self): return self._tables()[1]
    def GetScaleSigmaSquares(self): return self._tables()[2]
    def GetInverseScaleSigmaSquares(self): return self._tables()[3]
    @property
    def mnFeaturesPerLevel(self): return self._tables()[4]
    @property
    def umax(self): return self._tables()[5]

    def max_keypoints(self):
        return self._L.orbx_max_keypoints(self._h)

    # -- operator()
    def __call__(self, image):
        image = np.asarray(image)
        if image.size == 0:  # empty image: silent return (src/ORBextractor.cc:1046-1047)
            return np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8)
        assert image.dtype == np.uint8 and image.ndim == 2, "CV_8UC1 expected (:1050)"
        if image.strides[1] != 1 or image.strides[0] < image.shape[1]:
            image = np.ascontiguousarray(image)   # a row-strided view (ROI of a wider image) is passed as it is
        h, w = image.shape
        cap = max(self.nfeatures + 8 * self.nlevels, 64) + 260
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int(0)
        self._ck(self._L.orbx_extract(self._h, _p(image), w, h, image.strides[0], _p(kps), _p(desc), cap, C.byref(n)))
        self._shape = (h, w)
        return kps[:n.value].copy(), desc[:n.value].copy()

    def extract_batch(self, images):
        """Batched many-frame mode on host arrays [B,h,w]: list of (keypoints, descriptors)."""
        images = np.ascontiguousarray(images, dtype=np.uint8)
        B, h, w = images.shape
        cap = max(self.nfeatures + 8 * self.nlevels, 64) + 260
        kps = np.zeros((B, cap), KP_DTYPE)
        desc = np.zeros((B, cap, 32), np.uint8)
        n = np.zeros(B, np.int32)
        ptrs = (C.c_void_p * B)(*[images[b].ctypes.data for b in range(B)])
        self._ck(self._L.orbx_extract_batch(self._h, C.cast(ptrs, C.c_void_p), B, w, h, w, _p(kps), _p(desc), cap, _p(n)))
        self._shape = (h, w)
        return [(kps[b, :n[b]].copy(), desc[b, :n[b]].copy()) for b in range(B)]

    def extract_batch_device(self, d_imgs, B, w, h, stride, image_stride, d_kps, d_desc, d_counts, cap, stream=0):
        """Device-resident batched mode; all d_* are raw device pointers (ints)."""
        self._ck(self._L.orbx_extract_batch_device(self._h, d_imgs, B, w, h, stride, image_stride, d_kps, d_desc,
                                                 d_counts, cap, stream))
        self._shape = (h, w)

    def prefetch_batch_device(self, d_imgs, B, w, h, stride, image_stride, side_stream=0):
        """Start the pyramid of the NEXT batch now (orbx_extract_batch_device_prefetch): the images must be complete in HBM."""
        self._ck(self._L.orbx_extract_batch_device_prefetch(self._h, d_imgs, B, w, h, stride, image_stride, side_stream))

    def extract_batch_device_padded(self, d_level0, B, w, h, image_stride, d_kps, d_desc, d_counts, cap, stream=0):
        """extract_batch_device on images in the layout of level0_layout() (orbx_extract_batch_device_padded): level 0 is read in place,
        so the images must stay unchanged until the stereo matcher call that works on this call's pyramid has finished."""
        self._ck(self._L.orbx_extract_batch_device_padded(self._h, d_level0, B, w, h, image_stride, d_kps, d_desc, d_counts, cap, stream))
        self._shape = (h, w)

    def prefetch_batch_device_padded(self, d_level0, B, w, h, image_stride, side_stream=0):
        """prefetch_batch_device for images in the layout of level0_layout() (orbx_extract_batch_device_padded_prefetch)."""
        self._ck(self._L.orbx_extract_batch_device_padded_prefetch(self._h, d_level0, B, w, h, image_stride, side_stream))

    def level0_in_place(self):
        """Developer build: 1 iff the last extraction call read level 0 in place from the caller's images (orbx_debug_level0_in_place)."""
        rc = self._L.orbx_debug_level0_in_place(self._h)
        if rc < 0:
            self._ck(rc)
        return rc

    def side_stream(self):
        """hipStream_t of the handle's own side stream (orbx_side_stream)."""
        return self._L.orbx_side_stream(self._h)

    def stereo_frame(self, left, right, mbf, mb):
        """One stereo frame host to host in one call (orbx_stereo_frame): -> dict(kl, dl, kr, dr, uright, depth, nmatch)."""
        left = np.ascontiguousarray(left, np.uint8); right = np.ascontiguousarray(right, np.uint8)
        assert left.shape == right.shape and left.ndim == 2
        hgt, w = left.shape
        cap = (self.max_keypoints() if self._shape == (hgt, w) else self.nfeatures + 3 * self.nlevels + 8 * 64) + 8
        kl, kr = np.zeros(cap, KP_DTYPE), np.zeros(cap, KP_DTYPE)
        dl, dr = np.zeros((cap, 32), np.uint8), np.zeros((cap, 32), np.uint8)
        ur, dp = np.zeros(cap, np.float32), np.zeros(cap, np.float32)
        nl, nr, nm = C.c_int(), C.c_int(), C.c_int()
        self._ck(self._L.orbx_stereo_frame(self._h, _p(left), _p(right), w, hgt, w, float(mbf), float(mb), cap, _p(kl), _p(dl), C.byref(nl),
                                         _p(kr), _p(dr), C.byref(nr), _p(ur), _p(dp), C.byref(nm)))
        self._shape = (hgt, w)
        a, b = nl.value, nr.value
        return {"kl": kl[:a].copy(), "dl": dl[:a].copy(), "kr": kr[:b].copy(), "dr": dr[:b].copy(), "uright": ur[:a].copy(),
                "depth": dp[:a].copy(), "nmatch": nm.value}

    def rgbd_frame(self, img, depth, cam, depth_map_factor=1.0, rgb=True, cap=None):
        """One RGB-D frame host to host in one call (orbx_rgbd_frame): GrabImageRGBD's conversions + the RGB-D Frame constructor's
        feature part.  img: uint8 [h, w] (gray), [h, w, 3] or [h, w, 4] (rgb: channel 0 is red); depth: uint16 / float32 [h, w] or
        None (the monocular constructor's tail: uright = depth = -1); cam: RGBDCamera; depth_map_factor: mDepthMapFactor
        -> dict(kp, desc, kun, uright, depth)."""
        img = np.asarray(img)
        assert img.dtype == np.uint8 and (img.ndim == 2 or (img.ndim == 3 and img.shape[2] in (3, 4))), "CV_8UC1/3/4 expected"
        hgt, w = img.shape[:2]
        ch = 1 if img.ndim == 2 else img.shape[2]
        if img.size and (img.strides[-1] != 1 or (ch > 1 and img.strides[1] != ch) or img.strides[0] < w * ch):
            img = np.ascontiguousarray(img)   # (a row-strided view is passed as it is)
        dp_ptr, dtype, dstride = None, DEPTH_F32, 0
        if depth is not None:
            depth = np.asarray(depth)
            assert depth.shape == (hgt, w) and depth.dtype in _DEPTH_TYPES, "CV_16U / CV_32F depth of the image's size expected"
            if depth.strides[1] != depth.itemsize or depth.strides[0] < w * depth.itemsize:
                depth = np.ascontiguousarray(depth)
            dp_ptr, dtype, dstride = depth.ctypes.data, _DEPTH_TYPES[depth.dtype], depth.strides[0]
        if cap is None:
            cap = (self.max_keypoints() if self._shape == (hgt, w) else self.nfeatures + 3 * self.nlevels + 8 * 64) + 8
        kp, kun = np.zeros(cap, KP_DTYPE), np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        ur, dp = np.zeros(cap, np.float32), np.zeros(cap, np.float32)
        n = C.c_int()
        rc = self._L.orbx_rgbd_frame(self._h, _p(img) if img.size else None, ch, int(bool(rgb)), w, hgt, img.strides[0] if img.size else 0,
                                     dp_ptr, dtype, dstride, float(depth_map_factor), C.byref(cam), int(cap), _p(kp), _p(desc), C.byref(n),
                                     _p(kun), _p(ur), _p(dp))
        self._ck(rc)
        if img.size:
            self._shape = (hgt, w)
        a = n.value
        return {"kp": kp[:a].copy(), "desc": desc[:a].copy(), "kun": kun[:a].copy(), "uright": ur[:a].copy(), "depth": dp[:a].copy()}

    def stereo_frame_view(self, left, right, mbf, mb, shape=None, stride=None):
        """The latency form of stereo_frame (orbx_stereo_frame_view): no copy commands, results in the handle's pinned record.
        left / right: uint8 numpy arrays [h, w] (pageable: staged by the call), or objects with data_ptr() (torch tensors - pinned
        host or device memory), or raw addresses (then shape = (h, w)).  Returns dict(kl, dl, kr, dr, uright, depth, nmatch, view):
        numpy VIEWS of the pinned record (valid until the call after the next one on this handle) and the StereoView with the
        device pointers (d_kl, d_dl, d_uright, ...)."""
        def addr(a):
            if isinstance(a, int):
                return a, None
            if hasattr(a, "data_ptr"):
                return a.data_ptr(), tuple(a.shape)
            a = np.ascontiguousarray(a, np.uint8)
            return a.ctypes.data, a.shape, a
        la, ra = addr(left), addr(right)
        hgt, w = shape if shape is not None else la[1]
        v = StereoView()
        self._ck(self._L.orbx_stereo_frame_view(self._h, la[0], ra[0], w, hgt, w if stride is None else int(stride), float(mbf), float(mb), C.byref(v)))
        self._shape = (hgt, w)
        a, b = v.nl, v.nr
        view = lambda p, n, dt: np.frombuffer((C.c_char * (n * np.dtype(dt).itemsize)).from_address(p), dt) if n > 0 else np.zeros(0, dt)
        return {"kl": view(v.kl, a, KP_DTYPE), "dl": view(v.dl, a * 32, np.uint8).reshape(a, 32), "kr": view(v.kr, b, KP_DTYPE),
                "dr": view(v.dr, b * 32, np.uint8).reshape(b, 32), "uright": view(v.uright, a, np.float32),
                "depth": view(v.depth, a, np.float32), "nmatch": v.nmatch, "view": v}

    @staticmethod
    def _raw_image(a, name):
        """uint8 [h, w] or [h, w, 3|4] host array -> (array, channels, row stride in bytes); row-strided views are passed as they are."""
        a = np.asarray(a)
        assert a.dtype == np.uint8 and (a.ndim == 2 or (a.ndim == 3 and a.shape[2] in (3, 4))), name + ": CV_8UC1/3/4 expected"
        ch = 1 if a.ndim == 2 else a.shape[2]
        if a.size and (a.strides[-1] != 1 or (ch > 1 and a.strides[1] != ch) or a.strides[0] < a.shape[1] * ch):
            a = np.ascontiguousarray(a)
        return a, ch, (a.strides[0] if a.size else 0)

    def stereo_frame_rectified(self, rect_left, rect_right, left, right, mbf, mb, rgb=True):
        """stereo_frame on a RAW pair (orbx_stereo_frame_rectified): ros_stereo's remap of both images with the two StereoRectifier
        maps, GrabImageStereo's cvtColor for colour input, then extraction and ComputeStereoMatches.  left / right: uint8 [h, w] or
        [h, w, 3|4] with one row stride (rgb: channel 0 is red) -> dict(kl, dl, kr, dr, uright, depth, nmatch)."""
        left, ch, stride = self._raw_image(left, "left")
        right, chr_, stride_r = self._raw_image(right, "right")
        assert left.shape == right.shape and ch == chr_, "left and right differ in shape"
        if stride_r != stride:
            left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
            stride = left.strides[0] if left.size else 0
        hgt, w = left.shape[:2]
        cap = (self.max_keypoints() if self._shape == (hgt, w) else self.nfeatures + 3 * self.nlevels + 8 * 64) + 8
        kl, kr = np.zeros(cap, KP_DTYPE), np.zeros(cap, KP_DTYPE)
        dl, dr = np.zeros((cap, 32), np.uint8), np.zeros((cap, 32), np.uint8)
        ur, dp = np.zeros(cap, np.float32), np.zeros(cap, np.float32)
        nl, nr, nm = C.c_int(), C.c_int(), C.c_int()
        self._ck(self._L.orbx_stereo_frame_rectified(self._h, _rect_handle(rect_left), _rect_handle(rect_right),
                                                     _p(left) if left.size else None, _p(right) if right.size else None, ch,
                                                     int(bool(rgb)), w, hgt, stride, float(mbf), float(mb), cap, _p(kl), _p(dl),
                                                     C.byref(nl), _p(kr), _p(dr), C.byref(nr), _p(ur), _p(dp), C.byref(nm)))
        if left.size:
            self._shape = (hgt, w)
        a, b = nl.value, nr.value
        return {"kl": kl[:a].copy(), "dl": dl[:a].copy(), "kr": kr[:b].copy(), "dr": dr[:b].copy(), "uright": ur[:a].copy(),
                "depth": dp[:a].copy(), "nmatch": nm.value}

    def stereo_frame_view_rectified(self, rect_left, rect_right, left, right, mbf, mb, rgb=True, shape=None, channels=None, stride=None):
        """The latency form on a RAW pair (orbx_stereo_frame_view_rectified).  left / right: uint8 numpy arrays [h, w] / [h, w, 3|4]
        (pageable: staged by the call), objects with data_ptr() (torch tensors - pinned host or device memory, [h, w] or [h, w, c]),
        or raw addresses (then shape = (h, w) and channels).  Returns what stereo_frame_view returns."""
        def addr(a):
            if isinstance(a, int):
                return a, None, a
            if hasattr(a, "data_ptr"):
                return a.data_ptr(), tuple(a.shape), a
            a = np.ascontiguousarray(a, np.uint8)
            return a.ctypes.data, a.shape, a
        la, ra = addr(left), addr(right)
        shp = la[1]
        hgt, w = shape if shape is not None else shp[:2]
        ch = channels if channels is not None else (1 if shp is None or len(shp) == 2 else shp[2])
        v = StereoView()
        self._ck(self._L.orbx_stereo_frame_view_rectified(self._h, _rect_handle(rect_left), _rect_handle(rect_right), la[0], ra[0],
                                                          int(ch), int(bool(rgb)), w, hgt, w * ch if stride is None else int(stride),
                                                          float(mbf), float(mb), C.byref(v)))
        self._shape = (hgt, w)
        a, b = v.nl, v.nr
        view = lambda p, n, dt: np.frombuffer((C.c_char * (n * np.dtype(dt).itemsize)).from_address(p), dt) if n > 0 else np.zeros(0, dt)
        return {"kl": view(v.kl, a, KP_DTYPE), "dl": view(v.dl, a * 32, np.uint8).reshape(a, 32), "kr": view(v.kr, b, KP_DTYPE),
                "dr": view(v.dr, b * 32, np.uint8).reshape(b, 32), "uright": view(v.uright, a, np.float32),
                "depth": view(v.depth, a, np.float32), "nmatch": v.nmatch, "view": v}

    def set_pyramid_buffers(self, n):
        """2 (default) or 3 pyramid buffers (orbx_set_pyramid_buffers)."""
        self._ck(self._L.orbx_set_pyramid_buffers(self._h, int(n)))

    def side_stream_for(self, main_stream):
        """The side stream, probed (and replaced if need be) so that it does not share a hardware queue with main_stream."""
        return self._L.orbx_side_stream_for(self._h, main_stream)

    def stream_wait_fast_stage(self, stream):
        """Order `stream` behind the FAST stage of the last extraction call (orbx_stream_wait_fast_stage)."""
        self._ck(self._L.orbx_stream_wait_fast_stage(self._h, stream))

    # -- mvImagePyramid (include/ORBextractor.h:85)
    def pyramid_level(self, level, b=0, padded=False):
        w, h = C.c_int(), C.c_int()
        self._ck(self._L.orbx_pyramid_host(self._h, b, level, int(padded), None, 0, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.uint8)
        self._ck(self._L.orbx_pyramid_host(self._h, b, level, int(padded), _p(out), w.value, C.byref(w), C.byref(h)))
        return out

    @property
    def mvImagePyramid(self):
        return [self.pyramid_level(l) for l in range(self.nlevels)]

    def pyramid_device(self, level, b=0):
        ptr, w, h, s = C.c_void_p(), C.c_int(), C.c_int(), C.c_int()
        self._ck(self._L.orbx_pyramid_device(self._h, b, level, C.byref(ptr), C.byref(w), C.byref(h), C.byref(s)))
        return ptr.value, w.value, h.value, s.value

    # -- test / profiling hooks
    def debug_level_points(self, level, stage, b=0):
        self._hooks()
        n = C.c_int()
        self._ck(self._L.orbx_debug_level_points(self._h, b, level, stage, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 3), np.int32)
        if n.value:
            self._ck(self._L.orbx_debug_level_points(self._h, b, level, stage, _p(out), n.value, C.byref(n)))
        return out[:n.value]

    def fast_kernels(self, B):
        """names of the FAST kernel(s) a batch of B images of the planned size runs"""
        st, ce, ipl = C.c_int(0), C.c_int(0), C.c_int(0)
        self._ck(self._L.orbx_fast_kernels(self._h, int(B), C.byref(st), C.byref(ce), C.byref(ipl)))
        self.fast_images_per_launch = ipl.value
        return [n for n, f in (("k_fast_strips", st.value), ("k_fast_cells", ce.value)) if f]

    def octree_fallbacks(self, B=1):
        """[B, nlevels] int32: 1 where the last call's quad-tree of that (image, level) was redone by the exact form."""
        self._hooks()
        out = np.zeros((B, self.nlevels), np.int32)
        self._ck(self._L.orbx_debug_octree_fallbacks(self._h, _p(out), B * self.nlevels))
        return out

    def blurred_mask(self):
        """Levels of the last call that were blurred as a whole by k_blur_levels (bit l)."""
        m = C.c_uint()
        self._ck(self._L.orbx_debug_blurred_level(self._h, 0, 0, None, 0, C.byref(m)))
        return m.value

    def blurred_level(self, level, b=0):
        """Level `level` of image b after GaussianBlur(7x7, sigma 2) as k_blur_levels wrote it (levels in blurred_mask())."""
        self._hooks()
        w, h = C.c_int(), C.c_int()
        self._ck(self._L.orbx_pyramid_host(self._h, b, level, 0, None, 0, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.uint8)
        self._ck(self._L.orbx_debug_blurred_level(self._h, b, level, _p(out), w.value, None))
        return out

    def debug_blur_patches(self, image):
        """Test hook: extract one image and also return the 37x37 blurred block around every keypoint [N,37,37]."""
        self._hooks()
        self._ck(self._L.orbx_debug_blur_patches(self._h, 1, None, 0))
        try:
            k, d = self(image)
            out = np.zeros((max(len(k), 1), 37, 37), np.uint8)
            if len(k):
                self._ck(self._L.orbx_debug_blur_patches(self._h, 1, _p(out), len(k)))
        finally:
            self._L.orbx_debug_blur_patches(self._h, 0, None, 0)
        return k, d, out[:len(k)]

    def debug_last_plan(self):
        """Test hook: the launch plan chunk 0 of the last extraction call executed -> dict of CHUNK_PLAN_FIELDS (+ "nslice")."""
        self._hooks()
        out = np.zeros(len(CHUNK_PLAN_FIELDS) + 16, np.int32)
        self._ck(self._L.orbx_debug_last_plan(self._h, _p(out), len(out)))
        return _plan_dict(out)

    def set_profiling(self, mode=1):
        """0/False off, 1/True events at every stage boundary, 2 only around k_fast_cells (see orbx.h)."""
        self._ck(self._L.orbx_set_profiling(self._h, int(mode)))

    def stage_ms(self):
        """(average ms per call [pyramid, FAST, quad-tree, describe, total], calls averaged)"""
        ms = np.zeros(NUM_STAGES, np.float32)
        n = C.c_int(0)
        self._ck(self._L.orbx_get_stage_ms(self._h, _p(ms), C.byref(n)))
        return ms, n.value


def debug_features_in_area(kun, geom, x, y, r, min_level=-1, max_level=-1, device=0):
    """Test hook: Frame::GetFeaturesInArea as the matchers see it -> indices in the reference's order."""
    kun = np.ascontiguousarray(kun, KP_DTYPE)
    out = np.zeros(max(len(kun), 1), np.int32)
    n = C.c_int(0)
    _check(lib(True).orbm_debug_features_in_area(_p(kun), len(kun), C.byref(geom), float(x), float(y), float(r), int(min_level),
                                             int(max_level), _p(out), C.byref(n), int(device)), lib(True))
    return out[:n.value].copy()


def debug_match_path():
    """Test hook: what the last guided search of this thread ran in the developer build -> (resolver RES_*, fall-back FB_*, dynamic LDS)."""
    out = np.zeros(3, np.int64)
    _check(lib(True).orbm_debug_match_path(_p(out)), lib(True))
    return int(out[0]), int(out[1]), int(out[2])


def debug_resolve_plan(mode, m, n, device=0):
    """Test hook, launches nothing: the fast path's resolver for mode (0 map points, 1 last frame, 2 windows, 3 initialization), m queries
    and n keypoints -> (resolver RES_*, dynamic LDS, static LDS of that kernel, the device's LDS limit per workgroup)."""
    out = np.zeros(4, np.int64)
    _check(lib(True).orbm_debug_resolve_plan(int(mode), int(m), int(n), int(device), _p(out)), lib(True))
    return tuple(int(v) for v in out)


def _plan_dict(out):
    d = {k: int(v) for k, v in zip(CHUNK_PLAN_FIELDS, out)}
    d["nslice"] = tuple(int(v) for v in out[len(CHUNK_PLAN_FIELDS):])
    return d


def debug_plan_chunk(ncells=(), opt=None, **fields):
    """Test hook, no HIP call (works without a GPU): the launch rule on a PlanInput given as keywords of PLAN_INPUT_FIELDS (default 0),
    per-level `ncells` and `opt` = {option key: value} -> (status, dict of CHUNK_PLAN_FIELDS + "nslice")."""
    a = np.zeros(len(PLAN_INPUT_FIELDS) + 16 + 32, np.int32)
    for k, v in fields.items():
        a[PLAN_INPUT_FIELDS.index(k)] = int(v)
    a[len(PLAN_INPUT_FIELDS):len(PLAN_INPUT_FIELDS) + len(ncells)] = ncells
    for k, v in (opt or {}).items():
        a[len(PLAN_INPUT_FIELDS) + 16 + int(k)] = int(v)
    out = np.zeros(len(CHUNK_PLAN_FIELDS) + 16, np.int32)
    rc = lib(True).orbx_debug_plan_chunk(_p(a), len(a), _p(out), len(out))
    return rc, _plan_dict(out)


def debug_size_plan(nfeatures, scale_factor, nlevels, w, h, tile=0):
    """Test hook, no HIP call (works without a GPU): what the image size w x h decides for an extractor (csrc/orbx_size_plan.h) -> dict:
    status, message, the tables sf / isf / sig2 / isig2 / nfeat / umax and, for an accepted size, geom (LEVEL_GEOM_DTYPE[16]), tab (int32),
    the SIZE_PLAN_FIELDS, stripBase[17] and chains (int32 [2][8][8])."""
    L = lib(True)
    tables, nu = np.zeros((4, 16), np.float32), np.zeros(32, np.int32)
    geom, sc = np.zeros(16, LEVEL_GEOM_DTYPE), np.zeros(len(SIZE_PLAN_FIELDS) + 17 + 128, np.int64)
    tab = np.zeros(0, np.int32)
    for _ in range(2):   # the second call with room for the table words the first one counted
        rc = L.orbx_debug_size_plan(nfeatures, scale_factor, nlevels, w, h, tile, _p(tables), _p(nu), _p(geom), geom.nbytes, _p(tab), len(tab),
                                    _p(sc), len(sc))
        if rc != ORBX_OK or len(tab) == sc[SIZE_PLAN_FIELDS.index("tabWords")]:
            break
        tab = np.zeros(int(sc[SIZE_PLAN_FIELDS.index("tabWords")]), np.int32)
    d = dict(status=rc, message=L.orbx_last_error().decode() if rc else "", sf=tables[0], isf=tables[1], sig2=tables[2], isig2=tables[3],
             nfeat=nu[:16], umax=nu[16:])
    if rc == ORBX_OK:
        n = len(SIZE_PLAN_FIELDS)
        d.update({k: int(v) for k, v in zip(SIZE_PLAN_FIELDS, sc)}, geom=geom, tab=tab, stripBase=sc[n:n + 17].astype(np.int32),
                 chains=sc[n + 17:].astype(np.int32).reshape(2, 8, 8))
    return d


def debug_pyr_records(nfeatures=0, scale_factor=0.0, nlevels=0, w=0, h=0, extractor=None):
    """Test hook: k_pyr_level's column and band records (csrc/orbx_size_plan.h: plan_pyr_records).  Without `extractor` what the image size
    decides, no HIP call (works without a GPU); with a developer-build ORBextractor the records of its planned size read back from its device
    buffers.  -> dict: status, message and, for an accepted size, cols (uint32 [n, 4]: A, oa | ob << 8 | valid << 16, aa, ab), bands (uint32
    words), nxc[16], colOff[16], nbands[2][16], bandOff[2][16] ([0] the 8-row form, [1] the 16-row form; word offsets, -1 = not built)."""
    L = extractor._L if extractor is not None else lib(True)
    hh = extractor._h if extractor is not None else None
    idx = np.zeros(2 + 6 * 16, np.int32)
    cols, bands = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    for _ in range(2):   # the second call with room for the words the first one counted
        rc = L.orbx_debug_pyr_records(hh, int(nfeatures), float(scale_factor), int(nlevels), int(w), int(h), _p(cols), len(cols), _p(bands), len(bands),
                                      _p(idx), len(idx))
        if rc != ORBX_OK or (len(cols) == idx[0] and len(bands) == idx[1]):
            break
        cols, bands = np.zeros(int(idx[0]), np.uint32), np.zeros(int(idx[1]), np.uint32)
    d = dict(status=rc, message=L.orbx_last_error().decode() if rc else "")
    if rc == ORBX_OK:
        d.update(cols=cols.reshape(-1, 4), bands=bands, nxc=idx[2:18].copy(), colOff=idx[18:34].copy(), nbands=idx[34:66].reshape(2, 16).copy(),
                 bandOff=idx[66:98].reshape(2, 16).copy())
    return d


def debug_thread_scratch():
    """Test hook, no HIP call (works without a GPU): the calling thread's matcher scratch in the developer build -> dict of
    THREAD_SCRATCH_FIELDS."""
    out = np.zeros(len(THREAD_SCRATCH_FIELDS), np.int64)
    _check(lib(True).orbm_debug_thread_scratch(_p(out), len(out)), lib(True))
    return {k: int(v) for k, v in zip(THREAD_SCRATCH_FIELDS, out)}


def debug_set_alloc_fill(enable, word=0):
    """Test hook, no HIP call by itself: from now on every scratch block the developer build allocates (device and pinned) is filled with the
    32-bit `word` before anything else happens to it; enable = 0 switches that off.  Process-wide; either call restarts the statistics."""
    _check(lib(True).orbx_debug_set_alloc_fill(int(bool(enable)), int(word) & 0xFFFFFFFF), lib(True))


def debug_alloc_fill_stats():
    """Test hook: (blocks filled, bytes filled) since the last debug_set_alloc_fill."""
    out = np.zeros(2, np.int64)
    _check(lib(True).orbx_debug_alloc_fill_stats(_p(out)), lib(True))
    return int(out[0]), int(out[1])


def debug_stall_stream(stream, microseconds, device=0):
    """Test hook: hold `stream` (a raw hipStream_t, 0 = the default stream) back by a one-wave spin of 1 .. 50000 microseconds; launches
    nothing else and waits for nothing."""
    _check(lib(True).orbx_debug_stall_stream(int(stream) if stream else None, int(microseconds), int(device)), lib(True))


DEBUG_STREAM_FIELDS = ("main", "side0", "side1", "arena", "staging")


def debug_streams(extractor=None):
    """Test hook, no HIP call: raw hipStream_t values (0 = none) as a dict of DEBUG_STREAM_FIELDS - the own stream and the two side streams
    of `extractor` (a developer-build ORBextractor, or None), then the calling thread's matcher arena and staging-pair streams."""
    if extractor is not None:
        extractor._hooks()
    out = (C.c_void_p * 5)()
    _check(lib(True).orbx_debug_streams(extractor._h if extractor is not None else None, out, 5), lib(True))
    return {k: int(v or 0) for k, v in zip(DEBUG_STREAM_FIELDS, out)}


def debug_stereo_path():
    """Test hook: the last stereo matcher call of this thread in the developer build -> (useLds, bhShift, nbins, restarted)."""
    out = np.zeros(4, np.int32)
    _check(lib(True).orbm_debug_stereo_path(_p(out)), lib(True))
    return tuple(int(v) for v in out)


def debug_sincosf(angles, device=0):
    """Test hook: the device's cosf / sinf restatement -> (sin, cos) float32 arrays."""
    a = np.ascontiguousarray(angles, np.float32)
    s, c = np.zeros_like(a), np.zeros_like(a)
    _check(lib(True).orbx_debug_sincosf(_p(a), len(a), _p(s), _p(c), int(device)), lib(True))
    return s, c


def pack_records_device(d_kps, d_desc, d_uright, d_depth, d_counts, B, cap, d_records, stream=0):
    """One record per frame for the result all-gather (raw device pointers; layout in orbx.h / batching.py)."""
    _check(lib().orbx_pack_records_device(d_kps, d_desc, d_uright, d_depth, d_counts, B, cap, d_records, stream))


def stereo_batch_device(ex_left, ex_right, B, left_slot0, right_slot0, d_kl, d_dl, d_nl, d_kr, d_dr, d_nr, cap,
                        mbf, mb, d_uright, d_depth, d_nmatch, stream=0, prev=False):
    """Device-resident Frame::ComputeStereoMatches for B frames (raw device pointers).  prev: on the pyramids of the
    extraction call before the last one (orbm_stereo_batch_device_prev)."""
    L = ex_left._L   # (the handles belong to one build of the library)
    fn = L.orbm_stereo_batch_device_prev if prev else L.orbm_stereo_batch_device
    _check(fn(ex_left._h, ex_right._h, B, left_slot0, right_slot0, d_kl, d_dl, d_nl, d_kr, d_dr, d_nr, cap, float(mbf), float(mb),
              d_uright, d_depth, d_nmatch, stream), L)


def gray_from_color_device(d_color, B, w, h, channels, rgb, stride, image_stride, d_gray, gray_stride, gray_image_stride, stream=0):
    """cvtColor(RGB[A]/BGR[A]2GRAY) of B colour images in HBM (orbx_gray_from_color_device; raw device pointers)."""
    _check(lib().orbx_gray_from_color_device(d_color, int(B), int(w), int(h), int(channels), int(bool(rgb)), int(stride), int(image_stride),
                                             d_gray, int(gray_stride), int(gray_image_stride), stream))


def rgbd_batch_device(d_kps, d_counts, B, cap, d_depth, depth_type, w, h, depth_stride, depth_image_stride, depth_map_factor, cam,
                      d_kun, d_uright, d_depth_out, stream=0):
    """UndistortKeyPoints + ComputeStereoFromRGBD of B frames on the device outputs of extract_batch_device
    (orbm_rgbd_batch_device; raw device pointers, d_depth None / 0 = the monocular tail)."""
    _check(lib().orbm_rgbd_batch_device(d_kps, d_counts, int(B), int(cap), d_depth or None, int(depth_type), int(w), int(h),
                                        int(depth_stride), int(depth_image_stride), float(depth_map_factor), C.byref(cam), d_kun,
                                        d_uright, d_depth_out, stream))


class StereoRectifier:
    """One camera of a raw stereo rig: cv::initUndistortRectifyMap(K, D, R, P[:, :3], (w, h), CV_32FC1) on the device
    (orbx_rectifier_create; ros_stereo.cc:106-107).  K, R: 3x3; P: 3x3 or 3x4 (the first three columns are used); D: 4, 5 or 8
    coefficients.  Immutable; maps() returns (M1, M2) as float32 [h, w], info() the tile counts and device bytes."""

    def __init__(self, K, D, R, P, w, h, device=0):
        self._L = lib()
        self._r = None
        K = np.ascontiguousarray(np.asarray(K, np.float64).reshape(3, 3))
        R = np.ascontiguousarray(np.asarray(R, np.float64).reshape(3, 3))
        P = np.asarray(P, np.float64)
        assert P.shape in ((3, 3), (3, 4)), "P: 3x3 or 3x4"
        P = np.ascontiguousarray(P[:, :3])
        D = np.ascontiguousarray(np.asarray(D, np.float64).ravel())
        r = C.c_void_p()
        _check(self._L.orbx_rectifier_create(_p(K), _p(D) if D.size else None, int(D.size), _p(R), _p(P), int(w), int(h), int(device),
                                             C.byref(r)), self._L)
        self._r = r
        self.w, self.h, self.device = int(w), int(h), int(device)

    @property
    def handle(self):
        return self._r.value

    def maps(self):
        mx, my = np.zeros((self.h, self.w), np.float32), np.zeros((self.h, self.w), np.float32)
        _check(self._L.orbx_rectifier_maps(self._r, _p(mx), _p(my)), self._L)
        return mx, my

    def info(self):
        t, g, b = C.c_int(), C.c_int(), C.c_size_t()
        _check(self._L.orbx_rectifier_info(self._r, C.byref(t), C.byref(g), C.byref(b)), self._L)
        return {"tiles": t.value, "gather_tiles": g.value, "device_bytes": b.value}

    def close(self):
        if self._r:
            self._L.orbx_rectifier_destroy(self._r)
            self._r = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _rect_handle(r):
    return None if r is None else (r.handle if isinstance(r, StereoRectifier) else r)


def rectify_device(r0, r1, B0, d_src, B, sw, sh, channels, rgb, stride, image_stride, d_gray, gray_stride, gray_image_stride, stream=0):
    """remap(INTER_LINEAR) + RGB[A]/BGR[A]2GRAY of B raw images in HBM (orbx_rectify_device; raw device pointers): images [0, B0)
    through r0, [B0, B) through r1 (StereoRectifier or None where no image uses it)."""
    _check(lib().orbx_rectify_device(_rect_handle(r0), _rect_handle(r1), int(B0), d_src, int(B), int(sw), int(sh), int(channels),
                                     int(bool(rgb)), int(stride), int(image_stride), d_gray, int(gray_stride), int(gray_image_stride),
                                     stream), lib())


def cloud_capacity(w, h, step=3):
    """ceil(w / step) * ceil(h / step): the points one w x h keyframe can give (orbx_cloud_capacity)."""
    return lib().orbx_cloud_capacity(int(w), int(h), int(step))


class CloudMapper:
    """PointCloudMapping(resolution) on the device (orbx_cloudmapper_create; src/pointcloudmapping.cc:29-34, 83-127): generatePointCloud
    of RGB-D keyframes and the pcl::VoxelGrid filter saveOctomap runs on each.  leaf: the voxel's edge (System.cc passes 0.1); step:
    every step-th pixel of every step-th row; alpha: the a of every generated point.  Points are CLOUD_DTYPE rows."""

    def __init__(self, leaf=0.1, step=3, alpha=255, device=0):
        self._L = lib()
        self._m = None
        m = C.c_void_p()
        _check(self._L.orbx_cloudmapper_create(float(leaf), int(step), int(alpha), int(device), C.byref(m)), self._L)
        self._m = m
        self.leaf, self.step, self.alpha, self.device = float(np.float32(leaf)), int(step), int(alpha), int(device)

    def close(self):
        if self._m:
            self._L.orbx_cloudmapper_destroy(self._m)
            self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def capacity(self, w, h):
        return self._L.orbx_cloud_capacity(int(w), int(h), self.step)

    def generate_device(self, d_depth, depth_type, depth_stride, depth_image_stride, depth_map_factor, d_color, channels, color_stride,
                        color_image_stride, B, w, h, fx, fy, cx, cy, Twc, d_points, cap, d_counts, stream=0):
        """generatePointCloud of B keyframes in HBM (orbx_cloud_generate_device; raw device pointers).  Twc: host, B x 4 x 4 doubles
        (the inverse pose matrices); d_points [B][cap] CLOUD_DTYPE rows in scan order, d_counts [B] int32.  Asynchronous."""
        T = np.ascontiguousarray(np.asarray(Twc, np.float64).reshape(int(B), 16))
        _check(self._L.orbx_cloud_generate_device(self._m, d_depth, int(depth_type), int(depth_stride), int(depth_image_stride),
                                                  float(depth_map_factor), d_color, int(channels), int(color_stride),
                                                  int(color_image_stride), int(B), int(w), int(h), float(fx), float(fy), float(cx),
                                                  float(cy), _p(T), d_points, int(cap), d_counts, stream), self._L)

    def voxel_device(self, d_points, d_counts, B, cap, d_out, out_cap, d_out_counts, stream=0):
        """The voxel-grid centroid filter of B clouds in HBM (orbx_cloud_voxel_device; raw device pointers).  d_out_counts [B]: the
        voxels of each cloud, -1 where the grid overflows (PCL returns its input there).  Asynchronous."""
        _check(self._L.orbx_cloud_voxel_device(self._m, d_points, d_counts, int(B), int(cap), d_out, int(out_cap), d_out_counts, stream),
               self._L)

    def keyframe_cloud(self, color, depth, fx, fy, cx, cy, Twc, depth_map_factor=1.0, cap=None):
        """One keyframe host to host (orbx_keyframe_cloud).  color: uint8 [h, w, 3|4]; depth: uint16 / float32 [h, w]; Twc: 4 x 4
        doubles -> (raw, filtered) CLOUD_DTYPE arrays: generatePointCloud's cloud and what VoxelGrid makes of it."""
        color, ch, cstride = ORBextractor._raw_image(color, "color")
        assert ch in (3, 4), "CV_8UC3 / CV_8UC4 colour expected"
        depth = np.asarray(depth)
        hgt, w = color.shape[:2]
        assert depth.shape == (hgt, w) and depth.dtype in _DEPTH_TYPES, "CV_16U / CV_32F depth of the image's size expected"
        if depth.size and (depth.strides[1] != depth.itemsize or depth.strides[0] < w * depth.itemsize):
            depth = np.ascontiguousarray(depth)
        T = np.ascontiguousarray(np.asarray(Twc, np.float64).reshape(16))
        if cap is None:
            cap = max(self.capacity(w, hgt), 1)
        raw, out = np.zeros(cap, CLOUD_DTYPE), np.zeros(cap, CLOUD_DTYPE)
        nr, n = C.c_int(), C.c_int()
        _check(self._L.orbx_keyframe_cloud(self._m, _p(color) if color.size else None, ch, cstride, _p(depth) if depth.size else None,
                                           _DEPTH_TYPES[depth.dtype], depth.strides[0] if depth.size else 0, float(depth_map_factor), w,
                                           hgt, float(fx), float(fy), float(cx), float(cy), _p(T), int(cap), _p(raw), C.byref(nr), _p(out),
                                           C.byref(n)), self._L)
        return raw[:nr.value].copy(), out[:n.value].copy()

    @staticmethod
    def _xform(M):
        """None (the reference's axis swap) or a 4 x 4 float32 matrix -> the 16 floats orbx_octree_device reads, or None."""
        return None if M is None else np.ascontiguousarray(np.asarray(M, np.float32).reshape(16))

    def octree_device(self, d_points, d_counts, B, cap, M, resolution, d_data, data_cap, d_leaves, leaf_cap, d_info, stream=0):
        """The occupancy octree of a map in HBM (orbx_octree_device; raw device pointers): the union of B segments of CLOUD_DTYPE rows
        as voxel_device writes them -> d_data: the .bt file's data bytes, d_leaves (0: skipped): OCTREE_LEAF_DTYPE rows in preorder,
        d_info: one orbx_octree_info_t (OctreeInfo).  M: None for the reference's axis swap, or 4 x 4 floats.  Asynchronous."""
        M = self._xform(M)
        _check(self._L.orbx_octree_device(self._m, d_points, d_counts, int(B), int(cap), _p(M), float(resolution), d_data or None,
                                          int(data_cap), d_leaves or None, int(leaf_cap), d_info, stream), self._L)

    def octomap_bt(self, points, M=None, resolution=0.1):
        """saveOctomap's tree of a host map (orbx_octomap_bt): CLOUD_DTYPE rows -> (the bytes of the .bt file octomap::OcTree::writeBinary
        would write, info dict: points_in, points_dropped, cells, leaves, tree_size, data_bytes, overflow)."""
        points = np.ascontiguousarray(points, CLOUD_DTYPE)
        M = self._xform(M)
        n, info, nb = len(points), OctreeInfo(), C.c_size_t()
        out = np.empty(192 + 2 * n, np.uint8)   # room for 1 inner node per point (a surface has about a third); the exact size otherwise
        for _ in range(2):
            rc = self._L.orbx_octomap_bt(self._m, _p(points) if n else None, n, _p(M), float(resolution), _p(out), out.size,
                                         C.byref(nb), C.byref(info))
            if rc != ORBX_ERR_CAPACITY:
                break
            out = np.empty(nb.value, np.uint8)
        _check(rc, self._L)
        return out[:nb.value].tobytes(), info.as_dict()


def compute_stereo_matches(ex_left, ex_right, kl, dl, kr, dr, mbf, mb):
    """Frame::ComputeStereoMatches (src/Frame.cc:481-655) -> (mvuRight, mvDepth, nmatches).

    ex_left / ex_right must have just extracted the left / right image (their pyramids are
    read on the device)."""
    L = ex_left._L   # (the handles belong to one build of the library)
    kl = np.ascontiguousarray(kl, KP_DTYPE); kr = np.ascontiguousarray(kr, KP_DTYPE)
    dl = np.ascontiguousarray(dl, np.uint8); dr = np.ascontiguousarray(dr, np.uint8)
    ur = np.full(len(kl), -1, np.float32); dp = np.full(len(kl), -1, np.float32)
    n = C.c_int(0)
    _check(L.orbm_stereo(ex_left._h, ex_right._h, _p(kl), _p(dl), len(kl), _p(kr), _p(dr), len(kr),
                         float(mbf), float(mb), _p(ur), _p(dp), C.byref(n)), L)
    return ur, dp, n.value


class ORBmatcher:
    """Mirror of ORB_SLAM2::ORBmatcher for the hot routines (include/ORBmatcher.h:37-102)."""
    TH_LOW = 50
    TH_HIGH = 100
    HISTO_LENGTH = 30  # src/ORBmatcher.cc:37-39

    def __init__(self, nnratio=0.6, checkOri=True, device=0):
        self.mfNNratio = float(nnratio)
        self.mbCheckOrientation = bool(checkOri)
        self.device = int(device)

    @staticmethod
    def DescriptorDistance(a, b):
        a = np.ascontiguousarray(a, np.uint8); b = np.ascontiguousarray(b, np.uint8)
        assert a.size == 32 and b.size == 32
        return matcher_lib().orbm_hamming(_p(a), _p(b))

    def SearchForInitialization(self, k1, d1, k2, d2, geom2, vbPrevMatched, windowSize=10):
        """(src/ORBmatcher.cc:405-520) -> (nmatches, vnMatches12, vbPrevMatched')"""
        k1 = np.ascontiguousarray(k1, KP_DTYPE); k2 = np.ascontiguousarray(k2, KP_DTYPE)
        d1 = np.ascontiguousarray(d1, np.uint8); d2 = np.ascontiguousarray(d2, np.uint8)
        prev = np.ascontiguousarray(vbPrevMatched, np.float32).copy()
        m12 = np.full(len(k1), -1, np.int32)
        n = C.c_int(0)
        _check(matcher_lib().orbm_search_for_initialization(_p(k1), _p(d1), len(k1), _p(k2), _p(d2), len(k2), C.byref(geom2),
                                                    _p(prev), _p(m12), int(windowSize), self.mfNNratio,
                                                    int(self.mbCheckOrientation), self.device, C.byref(n)))
        return n.value, m12, prev

    def SearchByProjection(self, kun, desc, uright, geom, scale_factors, mps, mp_desc, frame_mp, ext_obs=None, th=1.0):
        """SearchByProjection(Frame&, vector<MapPoint*>&, th) (src/ORBmatcher.cc:45-129)
        -> (nmatches, frame_mp')"""
        kun = np.ascontiguousarray(kun, KP_DTYPE); desc = np.ascontiguousarray(desc, np.uint8)
        uright = np.ascontiguousarray(uright, np.float32); sf = np.ascontiguousarray(scale_factors, np.float32)
        mps = np.ascontiguousarray(mps, MP_DTYPE); mp_desc = np.ascontiguousarray(mp_desc, np.uint8)
        fm = np.ascontiguousarray(frame_mp, np.int32).copy()
        eo = None if ext_obs is None else np.ascontiguousarray(ext_obs, np.int32)
        n = C.c_int(0)
        _check(matcher_lib().orbm_search_by_projection_mp(_p(kun), _p(desc), _p(uright), len(kun), C.byref(geom), _p(sf),
                                                  len(sf), _p(mps), _p(mp_desc), len(mps), _p(fm), _p(eo), float(th),
                                                  self.mfNNratio, self.device, C.byref(n)))
        return n.value, fm

    def SearchByProjectionFrame(self, kun, desc, uright, geom, scale_factors, cam, Tcw_cur, Tcw_last, last, last_desc,
                                cur_mp, ext_obs=None, th=7.0, bMono=False):
        """SearchByProjection(Frame &cur, const Frame &last, th, bMono) (src/ORBmatcher.cc:1330-1472)
        -> (nmatches, cur_mp')"""
        kun = np.ascontiguousarray(kun, KP_DTYPE); desc = np.ascontiguousarray(desc, np.uint8)
        uright = np.ascontiguousarray(uright, np.float32); sf = np.ascontiguousarray(scale_factors, np.float32)
        last = np.ascontiguousarray(last, LASTPT_DTYPE); last_desc = np.ascontiguousarray(last_desc, np.uint8)
        Tc = np.ascontiguousarray(Tcw_cur, np.float32); Tl = np.ascontiguousarray(Tcw_last, np.float32)
        cm = np.ascontiguousarray(cur_mp, np.int32).copy()
        eo = None if ext_obs is None else np.ascontiguousarray(ext_obs, np.int32)
        n = C.c_int(0)
        _check(matcher_lib().orbm_search_by_projection_frame(_p(kun), _p(desc), _p(uright), len(kun), C.byref(geom), _p(sf),
                                                     len(sf), C.byref(cam), _p(Tc), _p(Tl), _p(last), _p(last_desc),
                                                     len(last), _p(cm), _p(eo), float(th), int(bMono),
                                                     int(self.mbCheckOrientation), self.device, C.byref(n)))
        return n.value, cm


def search_by_projection_frame_device(d_kun, d_desc, d_uright, n, geom, scale_factors, cam, Tcw_cur, Tcw_last, last, d_last_desc,
                                      cur_mp, ext_obs=None, th=7.0, bMono=False, check_orientation=True, device=0, stream=0):
    """orbm_search_by_projection_frame_device: d_* are raw device pointers (the extractor's / stereo matcher's outputs in HBM)
    -> (nmatches, cur_mp')"""
    sf = np.ascontiguousarray(scale_factors, np.float32)
    last = np.ascontiguousarray(last, LASTPT_DTYPE)
    Tc = np.ascontiguousarray(Tcw_cur, np.float32); Tl = np.ascontiguousarray(Tcw_last, np.float32)
    cm = np.ascontiguousarray(cur_mp, np.int32).copy()
    eo = None if ext_obs is None else np.ascontiguousarray(ext_obs, np.int32)
    nm = C.c_int(0)
    _check(matcher_lib().orbm_search_by_projection_frame_device(d_kun, d_desc, d_uright, int(n), C.byref(geom), _p(sf), len(sf), C.byref(cam),
                                                        _p(Tc), _p(Tl), _p(last), d_last_desc, len(last), _p(cm), _p(eo), float(th),
                                                        int(bMono), int(check_orientation), int(device), C.byref(nm), stream))
    return nm.value, cm


def search_local_points_device(d_kun, d_desc, d_uright, n, geom, sf, pts, mp_desc, Tcw, cam, viewing_cos_limit, thresholds, frame_mp,
                               ext_obs, th, nnratio, device=0, stream=0):
    """orbm_search_local_points_device -> (nmatches, frame_mp', projections)"""
    sf = np.ascontiguousarray(sf, np.float32)
    pts = np.ascontiguousarray(pts, WORLDPOINT_DTYPE); md = np.ascontiguousarray(mp_desc, np.uint8)
    T = np.ascontiguousarray(Tcw, np.float32); thr = np.ascontiguousarray(thresholds, np.float32)
    fm = np.ascontiguousarray(frame_mp, np.int32).copy()
    eo = None if ext_obs is None else np.ascontiguousarray(ext_obs, np.int32)
    proj = np.zeros(len(pts), MP_DTYPE)
    nm = C.c_int(0)
    _check(matcher_lib().orbm_search_local_points_device(d_kun, d_desc, d_uright, int(n), C.byref(geom), _p(sf), len(sf), _p(pts), _p(md),
                                                 len(pts), _p(T), C.byref(cam), float(viewing_cos_limit), _p(thr), _p(fm), _p(eo),
                                                 float(th), float(nnratio), int(device), C.byref(nm), _p(proj), stream))
    return nm.value, fm, proj


def _pose_info(rec):
    return {"correspondences": int(rec["correspondences"]), "bad": int(rec["bad"]), "rounds": int(rec["rounds"]),
            "iterations": [int(x) for x in rec["iterations"]], "trials": [int(x) for x in rec["trials"]],
            "t": np.array(rec["t"], np.float64), "q": np.array(rec["q"], np.float64)}


def _as_camera(cam):
    return cam if isinstance(cam, Camera) else Camera(*[float(c) for c in cam])


def pose_optimization(obs, cam, Tcw, outlier=None, device=0):
    """Optimizer::PoseOptimization (orbo_pose_optimization): obs [n] POSE_OBS_DTYPE (ur < 0: monocular), cam a Camera or
    (fx, fy, cx, cy, mbf, mb), Tcw the float 4x4, outlier [n] = mvbOutlier (only the entries with valid == 0 matter; default zeros)
    -> (Tcw_out [4, 4] float32, outlier' [n] uint8, ngood, info dict: correspondences, bad, rounds, iterations, trials, t, q)"""
    obs = np.ascontiguousarray(obs, POSE_OBS_DTYPE)
    n = len(obs)
    T = np.ascontiguousarray(Tcw, np.float32).reshape(4, 4)
    To = np.zeros((4, 4), np.float32)
    out = np.zeros(n, np.uint8) if outlier is None else np.ascontiguousarray(outlier, np.uint8).copy()
    assert len(out) == n
    info = np.zeros(1, POSE_INFO_DTYPE)
    ng = C.c_int(0)
    cam = _as_camera(cam)
    _check(matcher_lib().orbo_pose_optimization(_p(obs), n, C.byref(cam), _p(T), _p(To), _p(out), C.byref(ng), _p(info), int(device)))
    return To, out, ng.value, _pose_info(info[0])


def pose_optimization_batch(obs, offsets, cams, Tcw, outlier=None, device=0):
    """orbo_pose_optimization_batch: B problems in one launch.  obs / outlier are the problems' entries back to back, offsets [B + 1]
    into them, cams B cameras, Tcw [B, 4, 4] -> (Tcw_out [B, 4, 4], outlier', ngood [B], infos: list of B dicts)"""
    obs = np.ascontiguousarray(obs, POSE_OBS_DTYPE)
    off = np.ascontiguousarray(offsets, np.int32)
    B = len(off) - 1
    T = np.ascontiguousarray(Tcw, np.float32).reshape(B, 4, 4)
    To = np.zeros((B, 4, 4), np.float32)
    out = np.zeros(len(obs), np.uint8) if outlier is None else np.ascontiguousarray(outlier, np.uint8).copy()
    assert len(out) == len(obs) and len(cams) == B
    cs = (Camera * max(B, 1))(*[_as_camera(c) for c in cams])
    infos = np.zeros(max(B, 1), POSE_INFO_DTYPE)
    ng = np.zeros(max(B, 1), np.int32)
    _check(matcher_lib().orbo_pose_optimization_batch(_p(obs), _p(off), B, C.addressof(cs), _p(T), _p(To), _p(out), _p(ng), _p(infos),
                                                      int(device)))
    return To, out, ng[:B], [_pose_info(infos[b]) for b in range(B)]


def pose_optimization_device(d_kun, d_uright, n, inv_level_sigma2, pts, cam, Tcw, outlier=None, device=0, stream=None):
    """orbo_pose_optimization_device: d_kun / d_uright are raw device pointers to the frame's undistorted keypoints and mvuRight
    (the extractor's / stereo matcher's outputs in HBM), pts [n] POSE_WORLDPOS_DTYPE the map-point positions
    -> (Tcw_out, outlier', ngood, info) as pose_optimization"""
    is2 = np.ascontiguousarray(inv_level_sigma2, np.float32)
    pts = np.ascontiguousarray(pts, POSE_WORLDPOS_DTYPE)
    assert len(pts) == n
    T = np.ascontiguousarray(Tcw, np.float32).reshape(4, 4)
    To = np.zeros((4, 4), np.float32)
    out = np.zeros(n, np.uint8) if outlier is None else np.ascontiguousarray(outlier, np.uint8).copy()
    info = np.zeros(1, POSE_INFO_DTYPE)
    ng = C.c_int(0)
    cam = _as_camera(cam)
    _check(matcher_lib().orbo_pose_optimization_device(d_kun, d_uright, int(n), _p(is2), len(is2), _p(pts), C.byref(cam), _p(T), _p(To),
                                                       _p(out), C.byref(ng), _p(info), int(device), stream or None))
    return To, out, ng.value, _pose_info(info[0])


def sim3opt_problem(Tcw1, Tcw2, K1, K2, R, t, s, th2, fix_scale):
    """one SIM3OPT_PROBLEM_DTYPE record: the keyframes' float 4x4 poses, K = (fx, fy, cx, cy) of each, Sim3Solver's R / t / s, the
    chi2 threshold and bFixScale"""
    p = np.zeros(1, SIM3OPT_PROBLEM_DTYPE)
    p["Tcw1"], p["Tcw2"] = np.asarray(Tcw1, np.float32).reshape(16), np.asarray(Tcw2, np.float32).reshape(16)
    p["K1"], p["K2"] = np.asarray(K1, np.float32)[:4], np.asarray(K2, np.float32)[:4]
    p["R"], p["t"], p["s"] = np.asarray(R, np.float32).reshape(9), np.asarray(t, np.float32).reshape(3), s
    p["th2"], p["fix_scale"] = th2, int(bool(fix_scale))
    return p[0]


def _sim3opt_info(rec):
    return {"correspondences": int(rec["correspondences"]), "bad": int(rec["bad"]), "rounds": int(rec["rounds"]),
            "iterations": [int(x) for x in rec["iterations"]], "trials": [int(x) for x in rec["trials"]],
            "q": np.array(rec["q"], np.float64), "t": np.array(rec["t"], np.float64), "s": float(rec["s"])}


def optimize_sim3(matches, problem, device=0):
    """Optimizer::OptimizeSim3 (orbz_optimize_sim3): matches [n] SIM3OPT_MATCH_DTYPE (the rows the reference's filter accepts), problem
    one SIM3OPT_PROBLEM_DTYPE record (sim3opt_problem) -> (S12 [4, 4] float32 = s*R | t, dropped [n] uint8, ninliers, info dict:
    correspondences, bad, rounds, iterations, trials, q (x y z w), t, s in double).  rounds < 2: the reference's early `return 0` -
    the first round's drops, the Sim3 as it came in."""
    m = np.ascontiguousarray(matches, SIM3OPT_MATCH_DTYPE)
    n = len(m)
    pr = np.ascontiguousarray(np.asarray(problem, SIM3OPT_PROBLEM_DTYPE).reshape(1))
    So = np.zeros((4, 4), np.float32)
    dropped = np.zeros(n, np.uint8)
    info = np.zeros(1, SIM3OPT_INFO_DTYPE)
    ni = C.c_int(0)
    _check(matcher_lib().orbz_optimize_sim3(_p(m), n, _p(pr), _p(So), _p(dropped), C.byref(ni), _p(info), int(device)))
    return So, dropped, ni.value, _sim3opt_info(info[0])


def optimize_sim3_batch(matches, offsets, problems, device=0):
    """orbz_optimize_sim3_batch: B problems (loop candidates) in one launch.  matches are the problems' rows back to back, offsets
    [B + 1] into them (offsets[0] need not be 0), problems [B] SIM3OPT_PROBLEM_DTYPE
    -> (S12 [B, 4, 4], dropped [len(matches)], ninliers [B], infos: list of B dicts)"""
    m = np.ascontiguousarray(matches, SIM3OPT_MATCH_DTYPE)
    off = np.ascontiguousarray(offsets, np.int32)
    B = len(off) - 1
    pr = np.ascontiguousarray(np.asarray(problems, SIM3OPT_PROBLEM_DTYPE).reshape(-1))
    assert len(pr) == B and (B == 0 or off[B] <= len(m))
    So = np.zeros((max(B, 1), 4, 4), np.float32)
    dropped = np.zeros(len(m), np.uint8)
    infos = np.zeros(max(B, 1), SIM3OPT_INFO_DTYPE)
    ni = np.zeros(max(B, 1), np.int32)
    _check(matcher_lib().orbz_optimize_sim3_batch(_p(m), _p(off), B, _p(pr), _p(So), _p(dropped), _p(ni), _p(infos), int(device)))
    return So[:B], dropped, ni[:B], [_sim3opt_info(infos[b]) for b in range(B)]


def lba_schedule(rounds=2, iterations=(5, 10), robust=(1, 0), delta_mono=None, delta_stereo=None, classify=1, check_stop_first=1):
    """one LBA_SCHEDULE_DTYPE record; the defaults are Optimizer::LocalBundleAdjustment's (src/Optimizer.cc:569-570, :655-707)"""
    s = np.zeros(1, LBA_SCHEDULE_DTYPE)
    s["rounds"], s["iterations"], s["robust"] = rounds, (list(iterations) + [0])[:2], (list(robust) + [0])[:2]
    s["delta_mono"] = np.float32(np.sqrt(5.991)) if delta_mono is None else delta_mono
    s["delta_stereo"] = np.float32(np.sqrt(7.815)) if delta_stereo is None else delta_stereo
    s["classify"], s["check_stop_first"] = int(bool(classify)), int(bool(check_stop_first))
    return s[0]


def _lba_run(call, keyframes, points, observations, stop, device, binfo=None):
    kf = np.ascontiguousarray(keyframes, LBA_KEYFRAME_DTYPE)
    pt = np.ascontiguousarray(points, LBA_POINT_DTYPE)
    ob = np.ascontiguousarray(observations, LBA_OBSERVATION_DTYPE)
    K, P, E = len(kf), len(pt), len(ob)
    To, Po, erase = np.zeros((K, 4, 4), np.float32), np.zeros((P, 3), np.float32), np.zeros(E, np.uint8)
    info, ke, pe = np.zeros(1, LBA_INFO_DTYPE), np.zeros((K, 7), np.float64), np.zeros((P, 3), np.float64)
    raised = []

    def poll(_user):
        try:
            return 1 if stop() else 0
        except BaseException as e:      # noqa: BLE001   an exception cannot cross the C frames: stop the optimisation, raise afterwards
            raised.append(e)
            return 1
    fn = LBA_STOP_FN(poll) if stop is not None else LBA_STOP_FN()
    rc = call(matcher_lib(), _p(kf), K, _p(pt), P, _p(ob), E, fn, _p(To), _p(Po), _p(erase), _p(info), _p(ke), _p(pe), int(device))
    if raised:
        raise raised[0]
    _check(rc)
    inf = {k: (int(info[0][k]) if info[0][k].ndim == 0 else [int(x) for x in info[0][k]]) for k in LBA_INFO_DTYPE.names}
    if binfo is not None:      # the blocked path's record, filled by the call
        inf.update({k: (int(binfo[0][k]) if binfo[0][k].ndim == 0 else [int(x) for x in binfo[0][k]]) for k in LBA_BLOCKED_INFO_DTYPE.names})
    return To, Po, erase, inf, ke, pe


def local_bundle_adjustment(keyframes, points, observations, stop=None, device=0):
    """Optimizer::LocalBundleAdjustment (orbb_local_bundle_adjustment).  keyframes [K] LBA_KEYFRAME_DTYPE (fixed != 0: a fixed camera,
    or the local keyframe with mnId == 0), points [P] LBA_POINT_DTYPE, observations [E] LBA_OBSERVATION_DTYPE in any order (ur < 0:
    monocular), stop: a callable polled where the reference reads pbStopFlag (or None)
    -> (Tcw [K, 4, 4] float32, points [P, 3] float32, erase [E] uint8, info dict, kf_est [K, 7] float64 (q = x y z w, then t),
    pt_est [P, 3] float64)."""
    return _lba_run(lambda L, kf, K, pt, P, ob, E, fn, To, Po, er, info, ke, pe, dev:
                    L.orbb_local_bundle_adjustment(kf, K, pt, P, ob, E, fn, None, To, Po, er, info, ke, pe, dev),
                    keyframes, points, observations, stop, device)


def bundle_adjustment(keyframes, points, observations, iterations=5, robust=True, stop=None, device=0):
    """Optimizer::BundleAdjustment (orbb_bundle_adjustment): one optimize(iterations), the Huber kernel iff robust, no classification
    -> as local_bundle_adjustment (erase is all zero).  Meant for the initial map: one workgroup factorises the reduced system.
    For a loop-closure-sized map call global_bundle_adjustment, the same arithmetic on the blocked path."""
    return _lba_run(lambda L, kf, K, pt, P, ob, E, fn, To, Po, er, info, ke, pe, dev:
                    L.orbb_bundle_adjustment(kf, K, pt, P, ob, E, int(iterations), int(bool(robust)), fn, None, To, Po, info, ke, pe, dev),
                    keyframes, points, observations, stop, device)


def global_bundle_adjustment(keyframes, points, observations, iterations=10, robust=False, stop=None, device=0):
    """Optimizer::GlobalBundleAdjustemnt of a loop-closure-sized map (orbb_global_bundle_adjustment; the defaults are
    LoopClosing::RunGlobalBundleAdjustment's): bundle_adjustment's schedule on the blocked reduced-system path - the Schur complement
    summed from the keyframe pairs that co-observe a point, the dense LDL^T blocked over the whole GPU
    -> as bundle_adjustment; info also carries blocks, panels, contributions (per round) and launches."""
    binfo = np.zeros(1, LBA_BLOCKED_INFO_DTYPE)
    return _lba_run(lambda L, kf, K, pt, P, ob, E, fn, To, Po, er, info, ke, pe, dev:
                    L.orbb_global_bundle_adjustment(kf, K, pt, P, ob, E, int(iterations), int(bool(robust)), fn, None, To, Po, info, ke, pe, _p(binfo), dev),
                    keyframes, points, observations, stop, device, binfo)


def bundle_adjustment_scheduled(keyframes, points, observations, schedule, stop=None, device=0, blocked=False):
    """orbb_optimize: the same kernels under a caller-given schedule (lba_schedule); blocked: orbb_optimize_blocked, the blocked
    reduced-system path (info then also carries blocks, panels, contributions and launches)"""
    sc = np.ascontiguousarray(np.asarray(schedule, LBA_SCHEDULE_DTYPE).reshape(1))
    if blocked:
        binfo = np.zeros(1, LBA_BLOCKED_INFO_DTYPE)
        return _lba_run(lambda L, kf, K, pt, P, ob, E, fn, To, Po, er, info, ke, pe, dev:
                        L.orbb_optimize_blocked(kf, K, pt, P, ob, E, _p(sc), fn, None, To, Po, er, info, ke, pe, _p(binfo), dev),
                        keyframes, points, observations, stop, device, binfo)
    return _lba_run(lambda L, kf, K, pt, P, ob, E, fn, To, Po, er, info, ke, pe, dev:
                    L.orbb_optimize(kf, K, pt, P, ob, E, _p(sc), fn, None, To, Po, er, info, ke, pe, dev),
                    keyframes, points, observations, stop, device)


def optimize_essential_graph(vertices, edges, points, fix_scale, iterations=20, device=0):
    """Optimizer::OptimizeEssentialGraph (orbg_optimize_essential_graph).  vertices [N] EG_VERTEX_DTYPE (Scw: the CorrectedSim3 entry or
    Sim3(Rcw, tcw, 1) of the pose; Snc with has_nc: the NonCorrectedSim3 entry; fixed: pLoopKF), edges [E] EG_EDGE_DTYPE
    (essential_graph_edges builds them), points [P] EG_POINT_DTYPE (ref: the vertex of mnCorrectedReference or of the reference keyframe)
    -> (Tcw [N, 4, 4] float32 = [R, t / s], points [P, 3] float32, est [N, 8] float64 (q = x y z w, t, s), info dict)."""
    vt = np.ascontiguousarray(vertices, EG_VERTEX_DTYPE)
    ed = np.ascontiguousarray(edges, EG_EDGE_DTYPE)
    pt = np.ascontiguousarray(points, EG_POINT_DTYPE)
    N, E, P = len(vt), len(ed), len(pt)
    To, Po, est, info = np.zeros((N, 4, 4), np.float32), np.zeros((P, 3), np.float32), np.zeros((N, 8), np.float64), np.zeros(1, EG_INFO_DTYPE)
    _check(matcher_lib().orbg_optimize_essential_graph(_p(vt), N, _p(ed), E, _p(pt), P, int(bool(fix_scale)), int(iterations), _p(To), _p(Po),
                                                       _p(est), _p(info), int(device)))
    inf = {k: (info[0][k].item() if info[0][k].ndim == 0 else [int(x) for x in info[0][k]]) for k in EG_INFO_DTYPE.names}
    return To, Po, est, inf


class CovisTable(C.Structure):
    """orbc_table_t; `keep` holds the arrays the pointers look into."""
    _fields_ = [("kf", C.c_void_p), ("K", C.c_int32), ("pts", C.c_void_p), ("P", C.c_int32), ("obs_off", C.c_void_p), ("obs", C.c_void_p),
                ("scale_factors", C.c_void_p), ("nlevels", C.c_int32)]


class CovisQueries(C.Structure):
    """orbc_queries_t"""
    _fields_ = [("query_kf", C.c_void_p), ("Q", C.c_int32), ("feat_off", C.c_void_p), ("feat", C.c_void_p)]


class CovisConnections(C.Structure):
    """orbc_connections_t"""
    _fields_ = [("th", C.c_int32), ("cap", C.c_int32), ("ids", C.c_void_p), ("weights", C.c_void_p), ("n", C.c_void_p), ("counters", C.c_void_p)]


class CovisCulling(C.Structure):
    """orbc_culling_t"""
    _fields_ = [("monocular", C.c_int32), ("th_obs", C.c_int32), ("n_mps", C.c_void_p), ("n_redundant", C.c_void_p), ("verdict", C.c_void_p),
                ("point_bad", C.c_void_p)]


def covis_table(keyframes, points, rows, scale_factors):
    """The observation table of the orbc_* entry points.  keyframes [K] COVIS_KEYFRAME_DTYPE in slot order, points [P] COVIS_POINT_DTYPE,
    rows: (point, kf, idx, octave, stereo) per observation in any order, scale_factors [nlevels] -> dict with the CSR arrays: a point's
    list is sorted by kf (the walk order of the reference's std::map).  Two rows of one point by one keyframe raise ValueError."""
    kf = np.ascontiguousarray(keyframes, COVIS_KEYFRAME_DTYPE)
    pt = np.ascontiguousarray(points, COVIS_POINT_DTYPE)
    r = np.asarray(rows, np.int64).reshape(-1, 5)
    if len(r) and (r[:, 0].min() < 0 or r[:, 0].max() >= len(pt)):
        raise ValueError("covis_table: a row names a point outside [0, %d)" % len(pt))
    order = np.lexsort((r[:, 1], r[:, 0]))
    r = r[order]
    if len(r) > 1 and ((r[1:, 0] == r[:-1, 0]) & (r[1:, 1] == r[:-1, 1])).any():
        raise ValueError("covis_table: a point is observed twice by one keyframe")
    obs = np.zeros(len(r), COVIS_OBSERVATION_DTYPE)
    obs["kf"], obs["idx"], obs["octave"], obs["stereo"] = r[:, 1], r[:, 2], r[:, 3], r[:, 4] != 0
    off = np.zeros(len(pt) + 1, np.int32)
    off[1:] = np.cumsum(np.bincount(r[:, 0], minlength=len(pt)))
    return {"kf": kf, "pts": pt, "obs_off": off, "obs": obs, "sf": np.ascontiguousarray(scale_factors, np.float32)}


def covis_queries(query_kf, features):
    """Query keyframes of an orbc_* call: query_kf [Q] slots, features: per query an array of COVIS_FEATURE_DTYPE in feature-slot order
    (GetMapPointMatches()) -> dict with query_kf, feat_off, feat."""
    qk = np.ascontiguousarray(query_kf, np.int32).reshape(-1)
    fs = [np.ascontiguousarray(f, COVIS_FEATURE_DTYPE).reshape(-1) for f in features]
    if len(fs) != len(qk):
        raise ValueError("covis_queries: %d feature arrays for %d queries" % (len(fs), len(qk)))
    off = np.zeros(len(qk) + 1, np.int32)
    off[1:] = np.cumsum([len(f) for f in fs])
    return {"query_kf": qk, "feat_off": off, "feat": np.concatenate(fs) if fs else np.zeros(0, COVIS_FEATURE_DTYPE)}


def covis_check(table, queries, culling=False):
    """The precondition of include/orbx.h that the library does not check: a query's feature that names point p has an observation of p
    by that keyframe; with culling also the converse for (kf, idx), and distinct queries.  Raises ValueError."""
    off, obs = table["obs_off"], table["obs"]
    P = len(table["pts"])
    for q, s in enumerate(queries["query_kf"]):
        f = queries["feat"][queries["feat_off"][q]:queries["feat_off"][q + 1]]
        for i in np.nonzero(f["point"] >= 0)[0]:
            p = int(f["point"][i])
            if p >= P:
                continue   # the library reports it
            if not (obs["kf"][off[p]:off[p + 1]] == s).any():
                raise ValueError("covisibility: query %d (slot %d): feature %d names point %d, which has no observation by that keyframe" % (q, s, i, p))
        if culling:
            mine = np.nonzero(obs["kf"] == s)[0]
            owner = np.searchsorted(off, mine, side="right") - 1
            for o, p in zip(mine, owner):
                i = int(obs["idx"][o])
                if i >= len(f) or f["point"][i] != p:
                    raise ValueError("covisibility: query %d (slot %d): point %d lists feature %d, which does not name it" % (q, s, p, i))


def _covis_c_table(t):
    return CovisTable(_p(t["kf"]), len(t["kf"]), _p(t["pts"]), len(t["pts"]), _p(t["obs_off"]), _p(t["obs"]), _p(t["sf"]), len(t["sf"]))


def _covis_c_queries(q):
    return CovisQueries(_p(q["query_kf"]), len(q["query_kf"]), _p(q["feat_off"]), _p(q["feat"]))


def covisibility(table, connections=None, culling=None, normals=False, check=True, device=0):
    """Any of the three covisibility results of one table with ONE upload (orbc_covisibility).  connections: dict(queries=covis_queries(..),
    th=15, cap=None (K), counters=False); culling: dict(queries=.., monocular=.., th_obs=3, point_bad=True); normals: bool.
    -> dict with "connections": (ids [Q, cap], weights [Q, cap] (-1 beyond n), n [Q], counters [Q, K] or None),
    "culling": (n_mps [Q], n_redundant [Q], verdict [Q], point_bad [P] or None), "normals": [P] COVIS_NORMAL_DTYPE - those asked for."""
    L = matcher_lib()
    ct = _covis_c_table(table)
    K, P = len(table["kf"]), len(table["pts"])
    out = {}
    cq = cc = kq = kc = None
    nrm = np.zeros(P, COVIS_NORMAL_DTYPE) if normals else None
    if connections is not None:
        q = connections["queries"]
        if check:
            covis_check(table, q)
        Q = len(q["query_kf"])
        cap = connections.get("cap")
        cap = K if cap is None else int(cap)
        ids, w, n = np.full((Q, max(cap, 0)), -1, np.int32), np.full((Q, max(cap, 0)), -1, np.int32), np.zeros(Q, np.int32)
        cnt = np.zeros((Q, K), np.int32) if connections.get("counters") else None
        cq, cc = _covis_c_queries(q), CovisConnections(int(connections.get("th", 15)), cap, _p(ids), _p(w), _p(n), _p(cnt))
        out["connections"] = (ids, w, n, cnt)
    if culling is not None:
        q = culling["queries"]
        if check:
            covis_check(table, q, culling=True)
        Q = len(q["query_kf"])
        nm, nr, v = np.zeros(Q, np.int32), np.zeros(Q, np.int32), np.zeros(Q, np.int32)
        pb = np.zeros(P, np.uint8) if culling.get("point_bad", True) else None
        kq, kc = _covis_c_queries(q), CovisCulling(int(bool(culling["monocular"])), int(culling.get("th_obs", 3)), _p(nm), _p(nr), _p(v), _p(pb))
        out["culling"] = (nm, nr, v, pb)
    _check(L.orbc_covisibility(C.addressof(ct), C.addressof(cq) if cq else None, C.addressof(cc) if cc else None, C.addressof(kq) if kq else None,
                               C.addressof(kc) if kc else None, _p(nrm), int(device)), L)
    if normals:
        out["normals"] = nrm
    return out


def update_connections(table, queries, th=15, cap=None, counters=False, check=True, device=0):
    """KeyFrame::UpdateConnections of the query keyframes (orbc_update_connections) -> (ids, weights, n, counters or None): row q holds the
    first min(n[q], cap) entries of mvpOrderedConnectedKeyFrames / mvOrderedWeights as slots, -1 beyond."""
    return covisibility(table, connections=dict(queries=queries, th=th, cap=cap, counters=counters), check=check, device=device)["connections"]


def keyframe_culling(table, queries, monocular, th_obs=3, point_bad=True, check=True, device=0):
    """LocalMapping::KeyFrameCulling over the queries in order (orbc_keyframe_culling) -> (n_mps, n_redundant, verdict, point_bad or None);
    verdict 1: SetBadFlag erased the keyframe, 2: mbToBeErased."""
    return covisibility(table, culling=dict(queries=queries, monocular=monocular, th_obs=th_obs, point_bad=point_bad), check=check, device=device)["culling"]


def update_normal_and_depth(table, device=0):
    """MapPoint::UpdateNormalAndDepth of every point (orbc_update_normal_and_depth) -> [P] COVIS_NORMAL_DTYPE."""
    return covisibility(table, normals=True, device=device)["normals"]


class MapCorrectLoopOut(C.Structure):      # orbr_loop_out_t
    _fields_ = [("corrected", C.c_void_p), ("non_corrected", C.c_void_p), ("Tiw_new16", C.c_void_p), ("Ow_new3", C.c_void_p), ("pos3", C.c_void_p),
                ("corrected_ref", C.c_void_p), ("normals", C.c_void_p)]


class MapCorrectSpreadIn(C.Structure):     # orbr_spread_in_t
    _fields_ = [("K", C.c_int32), ("Tcw16", C.c_void_p), ("TcwGBA16", C.c_void_p), ("kf_in_gba", C.c_void_p), ("child_off", C.c_void_p), ("child", C.c_void_p),
                ("origins", C.c_void_p), ("n_origins", C.c_int32), ("P", C.c_int32), ("pos3", C.c_void_p), ("posGBA3", C.c_void_p), ("pt_in_gba", C.c_void_p),
                ("ref_kf", C.c_void_p), ("bad", C.c_void_p)]


class MapCorrectSpreadOut(C.Structure):    # orbr_spread_out_t
    _fields_ = [("Tcw_new16", C.c_void_p), ("TcwGBA_out16", C.c_void_p), ("kf_marked", C.c_void_p), ("kf_reached", C.c_void_p), ("pos_out3", C.c_void_p), ("status", C.c_void_p),
                ("levels", C.c_int32)]


MAPCORRECT_SIM3_DTYPE = EG_SIM3_DTYPE      # orbg_sim3_t: the entries of CorrectedSim3 / NonCorrectedSim3


def correct_loop_map(table, queries, cur, Tiw, Scw, device=0):
    """LoopClosing::CorrectLoop's pose and point correction (src/LoopClosing.cc:444-525 without :524; orbr_correct_loop).  table:
    covis_table(..); queries: covis_queries(..) of the connected keyframes, slots strictly ascending; cur: the slot of mpCurrentKF, one
    of them; Tiw [Q, 4, 4]: GetPose() of each query; Scw: one MAPCORRECT_SIM3_DTYPE record, mg2oScw.
    -> dict: corrected, non_corrected [Q] MAPCORRECT_SIM3_DTYPE; Tiw_new [Q, 4, 4]; Ow_new [Q, 3]; pos [P, 3]; corrected_ref [P] (the
    owner's slot, -1: untouched); normals [P] COVIS_NORMAL_DTYPE (status MAPCORRECT_NORMAL_UNTOUCHED where no query owns the point)."""
    L = matcher_lib()
    ct, cq = _covis_c_table(table), _covis_c_queries(queries)
    Q, P = len(queries["query_kf"]), len(table["pts"])
    T = np.ascontiguousarray(Tiw, np.float32)
    if T.shape != (Q, 4, 4):
        raise ValueError("correct_loop_map: Tiw has shape %s for %d queries" % (T.shape, Q))
    S = np.ascontiguousarray(Scw, MAPCORRECT_SIM3_DTYPE).reshape(1)
    out = {"corrected": np.zeros(Q, MAPCORRECT_SIM3_DTYPE), "non_corrected": np.zeros(Q, MAPCORRECT_SIM3_DTYPE), "Tiw_new": np.zeros((Q, 4, 4), np.float32),
           "Ow_new": np.zeros((Q, 3), np.float32), "pos": np.zeros((P, 3), np.float32), "corrected_ref": np.full(P, -1, np.int32),
           "normals": np.zeros(P, COVIS_NORMAL_DTYPE)}
    co = MapCorrectLoopOut(*[_p(out[k]) for k in ("corrected", "non_corrected", "Tiw_new", "Ow_new", "pos", "corrected_ref", "normals")])
    _check(L.orbr_correct_loop(C.addressof(ct), C.addressof(cq), int(cur), _p(T), _p(S), C.addressof(co), int(device)), L)
    return out


def spread_global_ba(Tcw, TcwGBA, kf_in_gba, child_off, child, origins, pos, posGBA, pt_in_gba, ref_kf, bad, device=0):
    """What LoopClosing::RunGlobalBundleAdjustment does after the optimisation (src/LoopClosing.cc:685-746; orbr_spread_global_ba).
    Tcw, TcwGBA [K, 4, 4]; kf_in_gba [K]; child_off [K + 1] / child: GetChilds() as slots (localmap_graph builds them); origins:
    mvpKeyFrameOrigins as slots; pos, posGBA [P, 3]; pt_in_gba [P]; ref_kf [P] (-1: none); bad [P].
    -> dict: Tcw_new, TcwGBA [K, 4, 4]; kf_marked, kf_reached [K]; pos [P, 3]; status [P] (MAPCORRECT_SPREAD_*); levels: the launches over the tree."""
    L = matcher_lib()
    a = {"Tcw": np.ascontiguousarray(Tcw, np.float32), "TcwGBA": np.ascontiguousarray(TcwGBA, np.float32), "kf_in_gba": np.ascontiguousarray(kf_in_gba, np.uint8),
         "child_off": np.ascontiguousarray(child_off, np.int32), "child": np.ascontiguousarray(child, np.int32).reshape(-1),
         "origins": np.ascontiguousarray(origins, np.int32).reshape(-1), "pos": np.ascontiguousarray(pos, np.float32), "posGBA": np.ascontiguousarray(posGBA, np.float32),
         "pt_in_gba": np.ascontiguousarray(pt_in_gba, np.uint8), "ref_kf": np.ascontiguousarray(ref_kf, np.int32), "bad": np.ascontiguousarray(bad, np.uint8)}
    K, P = len(a["kf_in_gba"]), len(a["bad"])
    if a["Tcw"].shape != (K, 4, 4) or a["TcwGBA"].shape != (K, 4, 4) or len(a["child_off"]) != K + 1:
        raise ValueError("spread_global_ba: %d keyframes, poses %s / %s, %d child offsets" % (K, a["Tcw"].shape, a["TcwGBA"].shape, len(a["child_off"])))
    if a["pos"].shape != (P, 3) or a["posGBA"].shape != (P, 3) or len(a["pt_in_gba"]) != P or len(a["ref_kf"]) != P:
        raise ValueError("spread_global_ba: %d points, positions %s / %s" % (P, a["pos"].shape, a["posGBA"].shape))
    out = {"Tcw_new": np.zeros((K, 4, 4), np.float32), "TcwGBA": np.zeros((K, 4, 4), np.float32), "kf_marked": np.zeros(K, np.uint8), "kf_reached": np.zeros(K, np.uint8),
           "pos": np.zeros((P, 3), np.float32), "status": np.zeros(P, np.int32)}
    si = MapCorrectSpreadIn(K, _p(a["Tcw"]), _p(a["TcwGBA"]), _p(a["kf_in_gba"]), _p(a["child_off"]), _p(a["child"]), _p(a["origins"]), len(a["origins"]), P,
                            _p(a["pos"]), _p(a["posGBA"]), _p(a["pt_in_gba"]), _p(a["ref_kf"]), _p(a["bad"]))
    so = MapCorrectSpreadOut(_p(out["Tcw_new"]), _p(out["TcwGBA"]), _p(out["kf_marked"]), _p(out["kf_reached"]), _p(out["pos"]), _p(out["status"]), 0)
    _check(L.orbr_spread_global_ba(C.addressof(si), C.addressof(so), int(device)), L)
    out["levels"] = int(so.levels)
    return out


class LocalMapMap(C.Structure):       # orbt_map_t
    _fields_ = [("table", C.c_void_p), ("features", C.c_void_p), ("parent", C.c_void_p), ("cov_off", C.c_void_p), ("cov", C.c_void_p),
                ("child_off", C.c_void_p), ("child", C.c_void_p), ("views", C.c_void_p), ("desc", C.c_void_p)]


class LocalMapResult(C.Structure):    # orbt_local_t
    _fields_ = [("frame_points", C.c_void_p), ("holder", C.c_void_p), ("ext_obs", C.c_void_p), ("local_kf", C.c_void_p), ("local_pts", C.c_void_p),
                ("pts", C.c_void_p), ("mp_desc", C.c_void_p), ("n_local_kf", C.c_int32), ("n_local_pts", C.c_int32), ("info", C.c_int32 * 8)]


def localmap_graph(parent, covisibles, children):
    """The keyframe graph of LocalMap.set_map.  parent [K]: slot of GetParent() or -1; covisibles [K]: GetVectorCovisibleKeyFrames() as
    lists of slots in the ordered list's order; children [K]: GetChilds() as collections of slots (stored ascending)
    -> dict(parent, cov_off, cov, child_off, child)."""
    pa = np.ascontiguousarray(parent, np.int32).reshape(-1)
    if len(covisibles) != len(pa) or len(children) != len(pa):
        raise ValueError("localmap_graph: %d parents, %d covisible lists, %d child lists" % (len(pa), len(covisibles), len(children)))

    def csr(lists):
        off = np.zeros(len(lists) + 1, np.int32)
        off[1:] = np.cumsum([len(x) for x in lists])
        flat = [int(v) for x in lists for v in x]
        return off, np.array(flat, np.int32).reshape(len(flat))
    co, cv = csr([list(c) for c in covisibles])
    ho, ch = csr([sorted(int(v) for v in c) for c in children])
    return {"parent": pa, "cov_off": co, "cov": cv, "child_off": ho, "child": ch}


class LocalMap:
    """Tracking::UpdateLocalMap on a snapshot of the map that stays on the device (orbt_*).  set_map when the map changed, update once per
    tracked frame.  One object is used by one thread at a time."""

    def __init__(self, device=0):
        self._L = matcher_lib()
        h = C.c_void_p()
        _check(self._L.orbt_localmap_create(int(device), C.byref(h)), self._L)
        self._h, self.K, self.P = h, 0, 0

    def close(self):
        if self._h:
            self._L.orbt_localmap_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_map(self, table, features, graph, views, desc):
        """table: covis_table(..); features: covis_queries(arange(K), every keyframe's GetMapPointMatches()); graph: localmap_graph(..);
        views [P] LOCALMAP_VIEW_DTYPE; desc [P, 32] uint8."""
        views = np.ascontiguousarray(views, LOCALMAP_VIEW_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8)
        P = len(table["pts"])
        if len(views) != P or desc.size != 32 * P:
            raise ValueError("LocalMap.set_map: %d points, %d views, %d descriptor bytes" % (P, len(views), desc.size))
        g = {k: np.ascontiguousarray(graph[k], np.int32) for k in ("parent", "cov_off", "cov", "child_off", "child")}
        K = len(table["kf"])
        if len(g["parent"]) != K or len(g["cov_off"]) != K + 1 or len(g["child_off"]) != K + 1 or len(features["feat_off"]) != len(features["query_kf"]) + 1:
            raise ValueError("LocalMap.set_map: the graph's arrays do not have the table's %d keyframes" % K)
        if (K and (g["cov_off"][K] > len(g["cov"]) or g["child_off"][K] > len(g["child"]))) or (len(features["query_kf"]) and features["feat_off"][-1] > len(features["feat"])):
            raise ValueError("LocalMap.set_map: an offset array ends beyond its list")
        ct, cq = _covis_c_table(table), _covis_c_queries(features)
        m = LocalMapMap(C.addressof(ct), C.addressof(cq), _p(g["parent"]), _p(g["cov_off"]), _p(g["cov"]), _p(g["child_off"]), _p(g["child"]), _p(views), _p(desc))
        rc = self._L.orbt_localmap_set_map(self._h, C.addressof(m))
        k, p = C.c_int(), C.c_int()
        self._L.orbt_localmap_info(self._h, C.addressof(k), C.addressof(p), None, None, None)
        self.K, self.P = k.value, p.value
        _check(rc, self._L)

    def info(self):
        """-> dict(K, P, features, snapshot_bytes, device_bytes)"""
        k, p, f, sb, db = C.c_int(), C.c_int(), C.c_int64(), C.c_size_t(), C.c_size_t()
        _check(self._L.orbt_localmap_info(self._h, C.addressof(k), C.addressof(p), C.addressof(f), C.addressof(sb), C.addressof(db)), self._L)
        return {"K": k.value, "P": p.value, "features": f.value, "snapshot_bytes": sb.value, "device_bytes": db.value}

    def update(self, frame_points, prev_kf=None, max_keyframes=80, nbest=10):
        """One frame (orbt_update_local_map).  frame_points [N]: the point index of mCurrentFrame.mvpMapPoints[i] or -1; prev_kf: the previous
        local keyframes -> dict: frame_points, holder, ext_obs [N]; local_kf; local_pts; pts (WORLDPOINT_DTYPE) and mp_desc [m, 32], the arrays
        search_local_points takes; info (LOCALMAP_INFO_DTYPE record)."""
        fp = np.ascontiguousarray(frame_points, np.int32).reshape(-1)
        pk = np.ascontiguousarray(prev_kf if prev_kf is not None else [], np.int32).reshape(-1)
        N, K, P = len(fp), self.K, self.P
        o = {"frame_points": np.empty(N, np.int32), "holder": np.empty(N, np.int32), "ext_obs": np.empty(N, np.int32), "local_kf": np.empty(K, np.int32),
             "local_pts": np.empty(P, np.int32), "pts": np.empty(P, WORLDPOINT_DTYPE), "mp_desc": np.empty((P, 32), np.uint8)}
        r = LocalMapResult(_p(o["frame_points"]), _p(o["holder"]), _p(o["ext_obs"]), _p(o["local_kf"]), _p(o["local_pts"]), _p(o["pts"]), _p(o["mp_desc"]))
        _check(self._L.orbt_update_local_map(self._h, _p(fp), N, _p(pk), len(pk), int(max_keyframes), int(nbest), C.addressof(r)), self._L)
        nk, m = r.n_local_kf, r.n_local_pts
        o["local_kf"] = o["local_kf"][:nk]
        for k in ("local_pts", "pts", "mp_desc"):
            o[k] = o[k][:m]
        o["info"] = np.array([tuple(r.info)], LOCALMAP_INFO_DTYPE)[0]
        return o


def essential_graph_edges(mnid, bad, parent, children, loop_edges, covisibles, weight, loop_connections, cur, loop, min_feat=100):
    """The edges Optimizer::OptimizeEssentialGraph builds (src/Optimizer.cc:849-985), restated for flat inputs - a pure function, no
    device.  The keyframes are numbered as vpKFs lists them: mnid [K], bad [K]; parent [K]: an index or -1; children, loop_edges [K]:
    sets of indices; covisibles [K]: GetCovisiblesByWeight(min_feat) as lists of indices; weight(a, b): GetWeight; loop_connections:
    {index: set of indices}; cur, loop: pCurKF and pLoopKF.  Where the reference walks a std::set or std::map of pointers (an order
    that is the allocator's), this walks in ascending mnId.  A bad keyframe has no vertex and no edge: the reference would hand
    g2o a null vertex there (a bad keyframe has left the map by then).
    -> (vertex [K]: the dense vertex index or -1, edges EG_EDGE_DTYPE: the loop connections (kind 0) first, then per keyframe its
    spanning-tree edge, its loop edges and its covisibility edges (kind 1))."""
    K = len(mnid)
    bad = [bool(b) for b in bad]
    vertex, n = [-1] * K, 0
    for k in range(K):
        if not bad[k]:
            vertex[k] = n
            n += 1
    by_id = lambda idx: sorted(idx, key=lambda a: mnid[a])      # noqa: E731
    edges, inserted = [], set()
    for k in by_id(loop_connections):
        for c in by_id(loop_connections[k]):
            if (mnid[k] != mnid[cur] or mnid[c] != mnid[loop]) and weight(k, c) < min_feat:
                continue
            if bad[k] or bad[c]:
                continue
            edges.append((vertex[k], vertex[c], 0))
            inserted.add((min(mnid[k], mnid[c]), max(mnid[k], mnid[c])))
    for k in range(K):
        if bad[k]:
            continue
        par = parent[k]
        if par >= 0 and not bad[par]:
            edges.append((vertex[k], vertex[par], 1))
        for l in by_id(loop_edges[k]):
            if mnid[l] < mnid[k] and not bad[l]:
                edges.append((vertex[k], vertex[l], 1))
        for c in covisibles[k]:
            if c != par and c not in children[k] and c not in loop_edges[k]:
                if not bad[c] and mnid[c] < mnid[k]:
                    if (min(mnid[k], mnid[c]), max(mnid[k], mnid[c])) in inserted:
                        continue
                    edges.append((vertex[k], vertex[c], 1))
    return np.array(vertex, np.int32), (np.array(edges, EG_EDGE_DTYPE) if edges else np.zeros(0, EG_EDGE_DTYPE))


class NewPointsKeyframe(C.Structure):
    """orbl_keyframe_t"""
    _fields_ = [("view", C.c_void_p), ("kp", C.c_void_p), ("st", C.c_void_p), ("n", C.c_int32), ("scale_factors", C.c_void_p),
                ("level_sigma2", C.c_void_p)]


class NewPointsNeighbour(C.Structure):
    """orbl_neighbour_t"""
    _fields_ = [("kf", NewPointsKeyframe), ("c_desc", C.c_void_p), ("c_flags", C.c_void_p), ("node_qstart", C.c_void_p), ("q_items", C.c_void_p),
                ("node_cstart", C.c_void_p), ("c_items", C.c_void_p), ("nnodes", C.c_int32), ("F12", C.c_float * 9), ("ex", C.c_float),
                ("ey", C.c_float), ("median_depth2", C.c_float)]


NEWPOINT_MAX_NEIGHBOURS = 32


def newpoints_view(Tcw, K, mb, mbf, scale_factor, nlevels):
    """one NEWPOINT_VIEW_DTYPE record of a keyframe: its float 4x4 pose, K = (fx, fy, cx, cy), mb, mbf, mfScaleFactor and the number
    of levels; invfx = 1.0f / fx and Ow = -Rwc*tcw as KeyFrame::SetPose forms it (the product in double, negated, narrowed once)"""
    v = np.zeros(1, NEWPOINT_VIEW_DTYPE)
    T = np.asarray(Tcw, np.float32).reshape(4, 4)
    v["Tcw"] = T.reshape(16)
    R, t = T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64)
    v["Ow"] = (((R[0] * t[0] + R[1] * t[1]) + R[2] * t[2]) * -1.0).astype(np.float32)
    fx, fy, cx, cy = [np.float32(k) for k in np.asarray(K, np.float32)[:4]]
    v["fx"], v["fy"], v["cx"], v["cy"], v["invfx"], v["invfy"] = fx, fy, cx, cy, np.float32(1.0) / fx, np.float32(1.0) / fy
    v["mb"], v["mbf"], v["scale_factor"], v["nlevels"] = mb, mbf, scale_factor, nlevels
    return v[0]


def newpoints_keyframe(view, kp, st, scale_factors, level_sigma2):
    """one side of a triangulation: the view (newpoints_view), mvKeysUn as KP_DTYPE, the stereo array (NEWPOINT_STEREO_DTYPE: mvuRight,
    mvDepth and the raw mvKeys position; None for a monocular keyframe; ur < 0 marks a monocular feature) and the level tables
    mvScaleFactors / mvLevelSigma2 -> a dict that keeps the contiguous arrays alive and holds the orbl_keyframe_t"""
    k = {"view": np.ascontiguousarray(np.asarray(view, NEWPOINT_VIEW_DTYPE).reshape(1)), "kp": np.ascontiguousarray(kp, KP_DTYPE),
         "st": None if st is None else np.ascontiguousarray(st, NEWPOINT_STEREO_DTYPE),
         "sf": np.ascontiguousarray(scale_factors, np.float32), "sig2": np.ascontiguousarray(level_sigma2, np.float32)}
    nl = int(k["view"]["nlevels"][0])
    assert k["st"] is None or len(k["st"]) == len(k["kp"])
    assert len(k["sf"]) >= min(max(nl, 0), NEWPOINT_MAX_LEVELS) and len(k["sig2"]) >= min(max(nl, 0), NEWPOINT_MAX_LEVELS)
    k["c"] = NewPointsKeyframe(_p(k["view"]), _p(k["kp"]), _p(k["st"]), len(k["kp"]), _p(k["sf"]), _p(k["sig2"]))
    return k


def triangulate_new_points(kf1, kf2, pairs, device=0):
    """The body of LocalMapping::CreateNewMapPoints for one pair of keyframes (orbl_triangulate): kf1 the current keyframe, kf2 the
    neighbour (newpoints_keyframe), pairs [nm, 2] the (idx1, idx2) SearchForTriangulation returned
    -> (points [nm] NEWPOINT_DTYPE, nnew).  status >= 0: a new map point at x y z."""
    pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    pts = np.zeros(len(pr), NEWPOINT_DTYPE)
    nn = C.c_int(0)
    a, b = kf1, kf2
    _check(matcher_lib().orbl_triangulate(_p(a["view"]), _p(a["kp"]), _p(a["st"]), len(a["kp"]), _p(a["sf"]), _p(a["sig2"]), _p(b["view"]),
                                          _p(b["kp"]), _p(b["st"]), len(b["kp"]), _p(b["sf"]), _p(b["sig2"]), _p(pr), len(pr), _p(pts),
                                          C.byref(nn), int(device)))
    return pts, nn.value


def triangulate_new_points_batch(kf1s, kf2s, match_off, pairs, device=0):
    """orbl_triangulate_batch: len(kf1s) pairs of keyframes in one launch; pair p's matches are pairs[match_off[p]:match_off[p + 1]]
    -> (points [len(pairs)], nnew [npairs])"""
    off = np.ascontiguousarray(match_off, np.int32)
    npairs = len(off) - 1
    pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    assert len(kf1s) == npairs and len(kf2s) == npairs and (npairs == 0 or off[npairs] <= len(pr))
    A = (NewPointsKeyframe * max(npairs, 1))(*[k["c"] for k in kf1s])
    B = (NewPointsKeyframe * max(npairs, 1))(*[k["c"] for k in kf2s])
    pts = np.zeros(len(pr), NEWPOINT_DTYPE)
    nn = np.zeros(max(npairs, 1), np.int32)
    _check(matcher_lib().orbl_triangulate_batch(C.addressof(A), C.addressof(B), npairs, _p(off), _p(pr), _p(pts), _p(nn), int(device)))
    return pts, nn[:npairs]


def newpoints_neighbour(kf, c_desc, c_flags, node_qstart, q_items, node_cstart, c_items, F12, ex, ey, median_depth2=0.0):
    """a covisible neighbour of create_new_map_points: its keyframe (newpoints_keyframe) and what search_for_triangulation takes for its
    candidate side - descriptors, flags, the four node lists of the two keyframes' common vocabulary nodes, F12 (compute_f12) and the
    epipole - plus ComputeSceneMedianDepth(2) for the monocular baseline rule"""
    n = {"kf": kf, "cd": np.ascontiguousarray(c_desc, np.uint8), "cf": np.ascontiguousarray(c_flags, np.uint8),
         "nqs": np.ascontiguousarray(node_qstart, np.int32), "qi": np.ascontiguousarray(q_items, np.int32),
         "ncs": np.ascontiguousarray(node_cstart, np.int32), "ci": np.ascontiguousarray(c_items, np.int32)}
    assert len(n["cd"]) == len(kf["kp"]) and len(n["cf"]) == len(kf["kp"]) and len(n["nqs"]) == len(n["ncs"])
    F = np.ascontiguousarray(F12, np.float32).reshape(9)
    n["c"] = NewPointsNeighbour(kf["c"], _p(n["cd"]), _p(n["cf"]), _p(n["nqs"]), _p(n["qi"]), _p(n["ncs"]), _p(n["ci"]), len(n["nqs"]) - 1,
                                (C.c_float * 9)(*[float(x) for x in F]), float(ex), float(ey), float(median_depth2))
    return n


def create_new_map_points(cur, q_desc, q_flags, neighbours, monocular, max_dist=50, check_orientation=False, device=0):
    """LocalMapping::CreateNewMapPoints' loop over the neighbours in one stream-ordered submission (orbl_create_new_map_points): cur the
    current keyframe (newpoints_keyframe), q_desc [nq, 32], q_flags [nq] (bit 0: no map point yet, bit 1: stereo), neighbours a list of
    newpoints_neighbour in covisibility order.  Defaults: ORBmatcher(0.6, false) and TH_LOW, as the reference calls it.
    -> dict: match_q [nn, nq], points [nn, nq] NEWPOINT_DTYPE, nmatches, nnew [nn], skipped [nn] bool, q_flags [nq] after the last neighbour"""
    qd, qf = np.ascontiguousarray(q_desc, np.uint8), np.ascontiguousarray(q_flags, np.uint8)
    nq, nn = len(cur["kp"]), len(neighbours)
    assert len(qd) == nq and len(qf) == nq
    N = (NewPointsNeighbour * max(nn, 1))(*[n["c"] for n in neighbours])
    mq = np.zeros((nn, nq), np.int32)
    pts = np.zeros((nn, nq), NEWPOINT_DTYPE)
    nm, nw, sk, fo = np.zeros(max(nn, 1), np.int32), np.zeros(max(nn, 1), np.int32), np.zeros(max(nn, 1), np.uint8), np.zeros(max(nq, 1), np.uint8)
    _check(matcher_lib().orbl_create_new_map_points(C.addressof(cur["c"]), _p(qd), _p(qf), C.addressof(N), nn, int(bool(monocular)), int(max_dist),
                                                    int(bool(check_orientation)), _p(mq), _p(pts), _p(nm), _p(nw), _p(sk), _p(fo), int(device)))
    return {"match_q": mq, "points": pts, "nmatches": nm[:nn], "nnew": nw[:nn], "skipped": sk[:nn].astype(bool), "q_flags": fo[:nq]}


def compute_f12(Tcw1, K1, Tcw2, K2):
    """LocalMapping::ComputeF12 (orbl_compute_f12, host code): the float 4x4 poses and K = (fx, fy, cx, cy) of the two keyframes
    -> F12 [3, 3] float32, what orbm_search_for_triangulation takes"""
    T1, T2 = np.ascontiguousarray(Tcw1, np.float32).reshape(16), np.ascontiguousarray(Tcw2, np.float32).reshape(16)
    k1, k2 = np.ascontiguousarray(np.asarray(K1, np.float32)[:4]), np.ascontiguousarray(np.asarray(K2, np.float32)[:4])
    F = np.zeros((3, 3), np.float32)
    _check(matcher_lib().orbl_compute_f12(_p(T1), _p(k1), _p(T2), _p(k2), _p(F)))
    return F


def baseline_ok(view1, view2, monocular, median_depth2=0.0):
    """the baseline rule of CreateNewMapPoints (orbl_baseline_ok, host code): False = the neighbour is skipped"""
    a = np.ascontiguousarray(np.asarray(view1, NEWPOINT_VIEW_DTYPE).reshape(1))
    b = np.ascontiguousarray(np.asarray(view2, NEWPOINT_VIEW_DTYPE).reshape(1))
    rc = matcher_lib().orbl_baseline_ok(_p(a), _p(b), int(bool(monocular)), float(median_depth2))
    if rc < 0:
        _check(rc)
    return bool(rc)


def draw_sets(n, iterations, rng):
    """mvSets (src/Initializer.cc:78-97): per iteration 8 distinct indices < n, drawn without replacement - the drawn slot is
    overwritten by the last available index, which is dropped - from a numpy Generator instead of rand()."""
    if n < 8:
        raise ValueError("draw_sets: %d matches, 8 are needed" % n)
    sets = np.zeros((int(iterations), 8), np.int32)
    for it in range(int(iterations)):
        avail = list(range(n))
        for j in range(8):
            k = int(rng.integers(0, len(avail)))
            sets[it, j] = avail[k]
            avail[k] = avail[-1]
            avail.pop()
    return sets


def _init_info(rec):
    d = {k: (rec[k].copy() if rec[k].ndim else rec[k].item()) for k in INIT_INFO_DTYPE.names}
    d["H21"], d["F21"] = d["H21"].reshape(3, 3), d["F21"].reshape(3, 3)
    d["ngood"], d["cand_parallax"] = d["ngood"][:d["ncand"]], d["cand_parallax"][:d["ncand"]]
    return d


def _init_args(matches12, sets, iterations, rng):
    m = np.ascontiguousarray(matches12, np.int32).reshape(-1, 2)
    if sets is None:
        sets = draw_sets(len(m), iterations, rng)
    s = np.ascontiguousarray(sets, np.int32).reshape(-1, 8)
    return m, s


class Initializer:
    """ORB_SLAM2::Initializer (src/Initializer.cc) on the GPU: keys1 [n1, 2] the reference frame's undistorted keypoint positions,
    K (fx, fy, cx, cy).  matches12 [N, 2]: index pairs into keys1 / keys2 (mvMatches12); sets [iterations, 8]: indices into
    matches12 (mvSets), drawn by draw_sets from a generator seeded with 0 when None."""

    def __init__(self, keys1, K, sigma=1.0, iterations=200, device=0):
        self.keys1 = np.ascontiguousarray(keys1, np.float32).reshape(-1, 2)
        self.K = np.ascontiguousarray([float(k) for k in K], np.float32)
        assert len(self.K) == 4
        self.sigma, self.iterations, self.device = float(sigma), int(iterations), int(device)
        self.rng = np.random.default_rng(0)

    def initialize(self, keys2, matches12, sets=None, min_parallax=1.0, min_triangulated=50):
        """-> (ok, R21 [3, 3], t21 [3], P3D [N, 3], triangulated [N] uint8, info dict), P3D / triangulated in match order"""
        k2 = np.ascontiguousarray(keys2, np.float32).reshape(-1, 2)
        m, s = _init_args(matches12, sets, self.iterations, self.rng)
        N = len(m)
        R, t, P, tri = np.zeros((3, 3), np.float32), np.zeros(3, np.float32), np.zeros((max(N, 1), 3), np.float32), np.zeros(max(N, 1), np.uint8)
        info, ok = np.zeros(1, INIT_INFO_DTYPE), C.c_int(0)
        _check(matcher_lib().orbi_initialize(_p(self.keys1), len(self.keys1), _p(k2), len(k2), _p(m), N, _p(s), len(s), _p(self.K), self.sigma,
                                             float(min_parallax), int(min_triangulated), C.byref(ok), _p(R), _p(t), _p(P), _p(tri), _p(info),
                                             self.device))
        return bool(ok.value), R, t, P[:N], tri[:N], _init_info(info[0])

    def search(self, keys2, matches12, sets=None):
        """FindHomography + FindFundamental only -> (scores [2, iterations] (H, F), inliersH [N], inliersF [N], info dict)"""
        k2 = np.ascontiguousarray(keys2, np.float32).reshape(-1, 2)
        m, s = _init_args(matches12, sets, self.iterations, self.rng)
        N = len(m)
        sc, iH, iF = np.zeros((2, max(len(s), 1)), np.float32), np.zeros(max(N, 1), np.uint8), np.zeros(max(N, 1), np.uint8)
        info = np.zeros(1, INIT_INFO_DTYPE)
        _check(matcher_lib().orbi_search(_p(self.keys1), len(self.keys1), _p(k2), len(k2), _p(m), N, _p(s), len(s), self.sigma, _p(sc), _p(iH),
                                         _p(iF), _p(info), self.device))
        return sc, iH[:N], iF[:N], _init_info(info[0])


def initialize_device(d_keys1, n1, d_keys2, n2, matches12, sets, K, sigma=1.0, min_parallax=1.0, min_triangulated=50, device=0, stream=None):
    """orbi_initialize_device: d_keys1 / d_keys2 are raw device pointers to the two frames' keypoint records (mvKeysUn in HBM)
    -> as Initializer.initialize"""
    m, s = _init_args(matches12, sets, 0, None)
    N = len(m)
    K = np.ascontiguousarray([float(k) for k in K], np.float32)
    R, t, P, tri = np.zeros((3, 3), np.float32), np.zeros(3, np.float32), np.zeros((max(N, 1), 3), np.float32), np.zeros(max(N, 1), np.uint8)
    info, ok = np.zeros(1, INIT_INFO_DTYPE), C.c_int(0)
    _check(matcher_lib().orbi_initialize_device(d_keys1, int(n1), d_keys2, int(n2), _p(m), N, _p(s), len(s), _p(K), float(sigma),
                                                float(min_parallax), int(min_triangulated), C.byref(ok), _p(R), _p(t), _p(P), _p(tri),
                                                _p(info), int(device), stream or None))
    return bool(ok.value), R, t, P[:N], tri[:N], _init_info(info[0])


def sim3_iterations(n, probability=0.99, min_inliers=6, max_iterations=300):
    """orbs_sim3_iterations: what Sim3Solver::SetRansacParameters (src/Sim3Solver.cc:114-138) leaves in mRansacMaxIts for n
    correspondences; 0 when n < min_inliers (iterate answers bNoMore without looking).  Host code, no device."""
    return int(matcher_lib().orbs_sim3_iterations(int(n), float(probability), int(min_inliers), int(max_iterations)))


def sim3_draw_sets(n, iterations, rng):
    """the minimal sets of Sim3Solver::iterate (:163-177): per iteration 3 distinct indices < n, drawn without replacement - the
    drawn slot is overwritten by the last available index, which is dropped - from a numpy Generator instead of rand()."""
    if n < 3 and iterations > 0:
        raise ValueError("sim3_draw_sets: %d pairs, 3 are needed" % n)
    sets = np.zeros((int(iterations), 3), np.int32)
    for it in range(int(iterations)):
        avail = list(range(n))
        for j in range(3):
            k = int(rng.integers(0, len(avail)))
            sets[it, j] = avail[k]
            avail[k] = avail[-1]
            avail.pop()
    return sets


def sim3_problem(Tcw1, Tcw2, K1, K2, fix_scale, min_inliers):
    p = np.zeros(1, SIM3_PROBLEM_DTYPE)
    p["Tcw1"], p["Tcw2"] = np.asarray(Tcw1, np.float32).reshape(16), np.asarray(Tcw2, np.float32).reshape(16)
    p["K1"], p["K2"] = [float(k) for k in K1], [float(k) for k in K2]
    p["fix_scale"], p["min_inliers"] = int(bool(fix_scale)), int(min_inliers)
    return p


def _sim3_info(rec):
    d = {k: (rec[k].copy() if rec[k].ndim else rec[k].item()) for k in SIM3_INFO_DTYPE.names}
    d["R"], d["T12"] = d["R"].reshape(3, 3), d["T12"].reshape(4, 4)
    return d


def sim3_ransac_batch(pairs, offsets, problems, sets, set_offsets, device=0):
    """orbs_sim3_ransac_batch: B problems (loop candidates) in one chain of launches.  pairs [offsets[B]] SIM3_PAIR_DTYPE, problems
    [B] SIM3_PROBLEM_DTYPE (sim3_problem), sets [set_offsets[B], 3] indices into each problem's own pairs
    -> a list of B dicts: the fields of orbs_sim3_info_t, counts [its], models [its, 13] (s, R, t), flags [its, n], hit_inliers [n]"""
    pairs = np.ascontiguousarray(pairs, SIM3_PAIR_DTYPE)
    problems = np.ascontiguousarray(problems, SIM3_PROBLEM_DTYPE)
    off, soff = np.ascontiguousarray(offsets, np.int32), np.ascontiguousarray(set_offsets, np.int32)
    B = len(problems)
    if len(off) != B + 1 or len(soff) != B + 1:
        raise ValueError("sim3_ransac_batch: %d problems need %d offsets" % (B, B + 1))
    sets = np.ascontiguousarray(sets, np.int32).reshape(-1, 3)
    np_, nh = int(off[-1]), int(soff[-1])
    if len(pairs) < np_ or len(sets) < nh:
        raise ValueError("sim3_ransac_batch: the offsets reach beyond the pairs or the sets")
    nfl = sum(max(int(soff[b + 1] - soff[b]), 0) * max(int(off[b + 1] - off[b]), 0) for b in range(B))
    counts, models = np.zeros(max(nh, 1), np.int32), np.zeros((max(nh, 1), 13), np.float32)
    flags, hit, infos = np.zeros(max(nfl, 1), np.uint8), np.zeros(max(np_, 1), np.uint8), np.zeros(max(B, 1), SIM3_INFO_DTYPE)
    pp = pairs if len(pairs) else np.zeros(1, SIM3_PAIR_DTYPE)
    ss = sets if len(sets) else np.zeros((1, 3), np.int32)
    _check(matcher_lib().orbs_sim3_ransac_batch(_p(pp), _p(off), B, _p(problems), _p(ss), _p(soff), _p(counts), _p(models), _p(flags),
                                                _p(hit), _p(infos), int(device)))
    out, fb = [], 0
    for b in range(B):
        n, its = int(off[b + 1] - off[b]), int(soff[b + 1] - soff[b])
        d = _sim3_info(infos[b])
        d.update(counts=counts[soff[b]:soff[b + 1]].copy(), models=models[soff[b]:soff[b + 1]].copy(),
                 flags=flags[fb:fb + its * n].reshape(its, n).copy(), hit_inliers=hit[off[b]:off[b + 1]].copy())
        fb += its * n
        out.append(d)
    return out


class Sim3Solver:
    """ORB_SLAM2::Sim3Solver (src/Sim3Solver.cc) on the GPU, on flat arrays: pairs [n] SIM3_PAIR_DTYPE (the world positions of the two
    matched map points, mvLevelSigma2[octave] of their keypoints), Tcw1 / Tcw2 the two keyframes' poses, K1 / K2 (fx, fy, cx, cy).
    The first iterate / find after set_ransac_parameters runs ONE device call over all mRansacMaxIts sets (drawn by sim3_draw_sets
    from a generator seeded with 0 when sets is None); every iterate(k) then advances over the stored counts with the
    reference's semantics."""

    def __init__(self, pairs, Tcw1, Tcw2, K1, K2, fix_scale, device=0):
        self.pairs = np.ascontiguousarray(pairs, SIM3_PAIR_DTYPE)
        self.Tcw1, self.Tcw2 = np.asarray(Tcw1, np.float32).reshape(4, 4), np.asarray(Tcw2, np.float32).reshape(4, 4)
        self.K1, self.K2, self.fix_scale, self.device = tuple(K1), tuple(K2), bool(fix_scale), int(device)
        self.rng = np.random.default_rng(0)
        self.set_ransac_parameters()

    def set_ransac_parameters(self, probability=0.99, min_inliers=6, max_iterations=300):
        self.min_inliers = int(min_inliers)
        self.max_iterations = sim3_iterations(len(self.pairs), probability, min_inliers, max_iterations)
        self.iterations, self.best_inliers, self.best_iteration, self._trace = 0, 0, -1, None

    def problem(self):
        return sim3_problem(self.Tcw1, self.Tcw2, self.K1, self.K2, self.fix_scale, self.min_inliers)

    def draw(self, sets=None):
        """the sets of the one device call: the first max_iterations rows of `sets`, or drawn"""
        if sets is None:
            return sim3_draw_sets(len(self.pairs), self.max_iterations, self.rng)
        s = np.ascontiguousarray(sets, np.int32).reshape(-1, 3)
        if len(s) < self.max_iterations:
            raise ValueError("Sim3Solver: %d sets, %d iterations" % (len(s), self.max_iterations))
        return s[:self.max_iterations]

    def prime(self, trace):
        self._trace = trace

    def trace(self, sets=None):
        """-> dict: the device call's answer (counts [its], models [its, 13], flags [its, n], hit_iteration, best_iteration, ...)"""
        if self._trace is None:
            s = self.draw(sets)
            self._trace = sim3_ransac_batch(self.pairs, [0, len(self.pairs)], self.problem(), s, [0, len(s)], self.device)[0]
        return self._trace

    def iterate(self, k, sets=None):
        """-> (T12 [4, 4] or None, no_more, inliers [n] uint8, n_inliers): Sim3Solver::iterate (:140-207)"""
        n = len(self.pairs)
        inl = np.zeros(n, np.uint8)
        if n < self.min_inliers:
            return None, True, inl, 0
        tr = self.trace(sets)
        cur = 0
        while self.iterations < self.max_iterations and cur < k:
            cur += 1
            i = self.iterations
            self.iterations += 1
            c = int(tr["counts"][i])
            if c >= self.best_inliers:
                self.best_inliers, self.best_iteration = c, i
                if c > self.min_inliers:
                    return self.estimated_T12(), False, tr["flags"][i].copy(), c
        return None, self.iterations >= self.max_iterations, inl, 0

    def find(self, sets=None):
        return self.iterate(self.max_iterations, sets)

    def estimated(self):
        """-> (s, R [3, 3], t [3]) of the best iteration so far (GetEstimatedScale / Rotation / Translation)"""
        m = self._trace["models"][self.best_iteration]
        return float(m[0]), m[1:10].reshape(3, 3).copy(), m[10:13].copy()

    def estimated_T12(self):
        s, R, t = self.estimated()
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = (R.astype(np.float64) * np.float64(np.float32(s))).astype(np.float32)
        T[:3, 3] = t
        return T

    @staticmethod
    def iterate_all(solvers, sets=None):
        """prime several solvers (loop candidates) with ONE batched device call; sets: a list with one array (or None) per solver"""
        todo = [(i, s) for i, s in enumerate(solvers) if s._trace is None and len(s.pairs) >= s.min_inliers]
        if not todo:
            return
        drawn = [s.draw(None if sets is None else sets[i]) for i, s in todo]
        off = np.cumsum([0] + [len(s.pairs) for _, s in todo])
        soff = np.cumsum([0] + [len(d) for d in drawn])
        res = sim3_ransac_batch(np.concatenate([s.pairs for _, s in todo]), off, np.concatenate([s.problem() for _, s in todo]),
                                np.concatenate(drawn), soff, todo[0][1].device)
        for (_, s), r in zip(todo, res):
            s.prime(r)


def pnp_parameters(n, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4):
    """orbp_pnp_parameters: PnPsolver::SetRansacParameters (src/PnPsolver.cc:121-157) -> (adjusted min_inliers, adjusted
    max_iterations).  Host code, no device.  min_set != 4 raises (ORBX_ERR_ARG)."""
    a, b = C.c_int(0), C.c_int(0)
    _check(matcher_lib().orbp_pnp_parameters(int(n), float(probability), int(min_inliers), int(max_iterations), int(min_set),
                                             float(epsilon), C.byref(a), C.byref(b)))
    return a.value, b.value


def pnp_draw_sets(n, iterations, rng):
    """the minimal sets of PnPsolver::iterate (:188-201): per iteration 4 distinct indices < n, drawn without replacement - the
    drawn slot is overwritten by the last available index, which is dropped - from a numpy Generator instead of rand()."""
    if n < 4 and iterations > 0:
        raise ValueError("pnp_draw_sets: %d correspondences, 4 are needed" % n)
    sets = np.zeros((int(iterations), 4), np.int32)
    for it in range(int(iterations)):
        avail = list(range(n))
        for j in range(4):
            k = int(rng.integers(0, len(avail)))
            sets[it, j] = avail[k]
            avail[k] = avail[-1]
            avail.pop()
    return sets


def pnp_problem(K, th2, min_inliers, max_iterations, iterations_done=0, prior_best_inliers=0):
    p = np.zeros(1, PNP_PROBLEM_DTYPE)
    p["K"], p["th2"] = [float(k) for k in K], float(th2)
    p["min_inliers"], p["max_iterations"] = int(min_inliers), int(max_iterations)
    p["iterations_done"], p["prior_best_inliers"] = int(iterations_done), int(prior_best_inliers)
    return p


def pnp_ransac_batch(corrs, offsets, problems, sets, set_offsets, prior_best_flags=None, device=0):
    """orbp_pnp_ransac_batch: B problems (relocalisation candidates), one PnPsolver::iterate call each, in one chain of launches.
    corrs [offsets[B]] PNP_CORR_DTYPE, problems [B] PNP_PROBLEM_DTYPE (pnp_problem), sets [set_offsets[B], 4] indices into each
    problem's own correspondences, prior_best_flags [offsets[B]] or None
    -> a list of B dicts: the fields of orbp_pnp_info_t (Tcw, best_Tcw as [4, 4]), counts [its], models [its, 12] float64 (R, t),
    tcws [its, 4, 4], choices [its], flags [its, n], refined_counts [its + 1], inliers [n], best_flags [n]"""
    corrs = np.ascontiguousarray(corrs, PNP_CORR_DTYPE)
    problems = np.ascontiguousarray(problems, PNP_PROBLEM_DTYPE)
    off, soff = np.ascontiguousarray(offsets, np.int32), np.ascontiguousarray(set_offsets, np.int32)
    B = len(problems)
    if len(off) != B + 1 or len(soff) != B + 1:
        raise ValueError("pnp_ransac_batch: %d problems need %d offsets" % (B, B + 1))
    sets = np.ascontiguousarray(sets, np.int32).reshape(-1, 4)
    np_, nh = int(off[-1]), int(soff[-1])
    if len(corrs) < np_ or len(sets) < nh:
        raise ValueError("pnp_ransac_batch: the offsets reach beyond the correspondences or the sets")
    prior = None
    if prior_best_flags is not None:
        prior = np.ascontiguousarray(prior_best_flags, np.uint8)
        if len(prior) < np_:
            raise ValueError("pnp_ransac_batch: %d prior flags, %d correspondences" % (len(prior), np_))
    nfl = sum(max(int(soff[b + 1] - soff[b]), 0) * max(int(off[b + 1] - off[b]), 0) for b in range(B))
    counts, choices = np.zeros(max(nh, 1), np.int32), np.zeros(max(nh, 1), np.int32)
    models, tcws = np.zeros((max(nh, 1), 12), np.float64), np.zeros((max(nh, 1), 4, 4), np.float32)
    rcounts = np.full(max(nh, 0) + B + 1, -1, np.int32)
    flags, inl, best = np.zeros(max(nfl, 1), np.uint8), np.zeros(max(np_, 1), np.uint8), np.zeros(max(np_, 1), np.uint8)
    infos = np.zeros(max(B, 1), PNP_INFO_DTYPE)
    cc = corrs if len(corrs) else np.zeros(1, PNP_CORR_DTYPE)
    ss = sets if len(sets) else np.zeros((1, 4), np.int32)
    _check(matcher_lib().orbp_pnp_ransac_batch(_p(cc), _p(off), B, _p(problems), _p(ss), _p(soff), None if prior is None else _p(prior),
                                               _p(counts), _p(models), _p(tcws), _p(choices), _p(flags), _p(rcounts), _p(inl), _p(best),
                                               _p(infos), int(device)))
    out, fb = [], 0
    for b in range(B):
        n, its = int(off[b + 1] - off[b]), int(soff[b + 1] - soff[b])
        d = {k: (infos[b][k].copy() if infos[b][k].ndim else infos[b][k].item()) for k in PNP_INFO_DTYPE.names}
        d["Tcw"], d["best_Tcw"] = d["Tcw"].reshape(4, 4), d["best_Tcw"].reshape(4, 4)
        h = slice(soff[b], soff[b + 1])
        d.update(counts=counts[h].copy(), models=models[h].copy(), tcws=tcws[h].copy(), choices=choices[h].copy(),
                 flags=flags[fb:fb + its * n].reshape(its, n).copy(), refined_counts=rcounts[soff[b] + b:soff[b + 1] + b + 1].copy(),
                 inliers=inl[off[b]:off[b + 1]].copy(), best_flags=best[off[b]:off[b + 1]].copy())
        fb += its * n
        out.append(d)
    return out


class PnPsolver:
    """ORB_SLAM2::PnPsolver (src/PnPsolver.cc) on the GPU, on flat arrays: corrs [n] PNP_CORR_DTYPE (the world position of the matched
    map point, the undistorted keypoint, mvLevelSigma2[octave]), K (fx, fy, cx, cy).  Every iterate(k) is ONE device call over the
    max(max_iterations - iterations, k) sets the reference's loop may run (drawn at the call by pnp_draw_sets from a generator
    seeded with 0, or the first rows of `sets`); the best set, its count and pose and the iteration counter are carried from call
    to call as the reference's members are."""

    def __init__(self, corrs, K, device=0):
        self.corrs = np.ascontiguousarray(corrs, PNP_CORR_DTYPE)
        self.K, self.device = tuple(float(k) for k in K), int(device)
        self.rng = np.random.default_rng(0)
        self.iterations, self.best_inliers, self.best_flags, self.best_Tcw = 0, 0, None, None
        self.set_ransac_parameters()

    def set_ransac_parameters(self, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4, th2=5.991):
        self.min_inliers, self.max_iterations = pnp_parameters(len(self.corrs), probability, min_inliers, max_iterations, min_set, epsilon)
        self.th2 = float(th2)

    def problem(self):
        return pnp_problem(self.K, self.th2, self.min_inliers, self.max_iterations, self.iterations, self.best_inliers)

    def planned(self, k):
        """how many iterations a call iterate(k) may run: the loop's condition is mnIterations < mRansacMaxIts || nCurrent < k"""
        return 0 if len(self.corrs) < self.min_inliers else max(self.max_iterations - self.iterations, int(k))

    def draw(self, k, sets=None):
        its = self.planned(k)
        if sets is None:
            return pnp_draw_sets(len(self.corrs), its, self.rng)
        s = np.ascontiguousarray(sets, np.int32).reshape(-1, 4)
        if len(s) < its:
            raise ValueError("PnPsolver: %d sets, %d iterations" % (len(s), its))
        return s[:its]

    def absorb(self, r):
        """take one problem's answer of pnp_ransac_batch -> (Tcw [4, 4] or None, no_more, inliers [n] uint8, n_inliers)"""
        self.last = r
        self.iterations += r["iterations_run"]
        if r["best_iteration"] >= 0:
            self.best_Tcw = r["best_Tcw"].copy()
        self.best_inliers, self.best_flags = r["best_inliers"], r["best_flags"].copy()
        if r["pose"] == PNP_POSE_REFINED:
            return r["Tcw"].copy(), False, r["inliers"].copy(), r["refined_inliers"]
        if r["pose"] in (PNP_POSE_BEST, PNP_POSE_PRIOR_BEST):
            return self.best_Tcw.copy(), True, r["inliers"].copy(), r["best_inliers"]
        return None, bool(r["no_more"]), np.zeros(len(self.corrs), np.uint8), 0

    def iterate(self, k, sets=None):
        """-> (Tcw [4, 4] or None, no_more, inliers [n] uint8, n_inliers): PnPsolver::iterate (:165-258)"""
        n = len(self.corrs)
        if n < self.min_inliers:
            return None, True, np.zeros(n, np.uint8), 0
        s = self.draw(k, sets)
        r = pnp_ransac_batch(self.corrs, [0, n], self.problem(), s, [0, len(s)], self.best_flags, self.device)[0]
        return self.absorb(r)

    def find(self, sets=None):
        return self.iterate(self.max_iterations, sets)

    @staticmethod
    def iterate_all(solvers, k, sets=None):
        """iterate(k) of several solvers (the live candidates of a Relocalization pass) as ONE batched device call; sets: a list
        with one array (or None) per solver -> a list of iterate's tuples"""
        out = [None] * len(solvers)
        todo = []
        for i, s in enumerate(solvers):
            if len(s.corrs) < s.min_inliers:
                out[i] = (None, True, np.zeros(len(s.corrs), np.uint8), 0)
            else:
                todo.append((i, s))
        if todo:
            drawn = [s.draw(k, None if sets is None else sets[i]) for i, s in todo]
            off = np.cumsum([0] + [len(s.corrs) for _, s in todo])
            soff = np.cumsum([0] + [len(d) for d in drawn])
            prior = np.concatenate([np.zeros(len(s.corrs), np.uint8) if s.best_flags is None else s.best_flags for _, s in todo])
            res = pnp_ransac_batch(np.concatenate([s.corrs for _, s in todo]), off, np.concatenate([s.problem() for _, s in todo]),
                                   np.concatenate(drawn), soff, prior, todo[0][1].device)
            for (i, s), r in zip(todo, res):
                out[i] = s.absorb(r)
        return out


def match_windows(kun, desc, uright, geom, queries, query_desc, holder, ext_blocks=None, max_dist=100,
                  check_orientation=True, device=0, geom_assign=None):
    """orbm_match_windows: the projected-window matcher behind the SearchByProjection family
    -> (nmatches, holder')"""
    kun = np.ascontiguousarray(kun, KP_DTYPE); desc = np.ascontiguousarray(desc, np.uint8)
    ur = None if uright is None else np.ascontiguousarray(uright, np.float32)
    q = np.ascontiguousarray(queries, WINDOW_DTYPE); qd = np.ascontiguousarray(query_desc, np.uint8)
    h = np.ascontiguousarray(holder, np.int32).copy()
    eb = None if ext_blocks is None else np.ascontiguousarray(ext_blocks, np.int32)
    n = C.c_int(0)
    _check(matcher_lib().orbm_match_windows(_p(kun), _p(desc), _p(ur), len(kun), C.byref(geom),
                                    None if geom_assign is None else C.byref(geom_assign), _p(q), _p(qd), len(q), _p(h),
                                    _p(eb), int(max_dist), int(check_orientation), int(device), C.byref(n)))
    return n.value, h


def best_in_windows(kun, desc, uright, geom, queries, query_desc, inv_level_sigma2=None, device=0, geom_assign=None):
    """orbm_best_in_windows: stateless window search behind Fuse / SearchBySim3 -> (best_idx, best_dist)"""
    kun = np.ascontiguousarray(kun, KP_DTYPE); desc = np.ascontiguousarray(desc, np.uint8)
    ur = None if uright is None else np.ascontiguousarray(uright, np.float32)
    q = np.ascontiguousarray(queries, WINDOW_DTYPE); qd = np.ascontiguousarray(query_desc, np.uint8)
    s2 = None if inv_level_sigma2 is None else np.ascontiguousarray(inv_level_sigma2, np.float32)
    bi = np.full(len(q), -1, np.int32); bd = np.full(len(q), 256, np.int32)
    _check(matcher_lib().orbm_best_in_windows(_p(kun), _p(desc), _p(ur), len(kun), C.byref(geom),
                                      None if geom_assign is None else C.byref(geom_assign), _p(q), _p(qd), len(q), _p(s2),
                                      0 if s2 is None else len(s2), _p(bi), _p(bd), int(device)))
    return bi, bd


def distinctive_descriptors(desc, offsets, device=0):
    """orbm_distinctive_descriptors: MapPoint::ComputeDistinctiveDescriptors batched -> (best_row, best_median)"""
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    off = np.ascontiguousarray(offsets, np.int32)
    m = len(off) - 1
    br = np.zeros(m, np.int32); bm = np.zeros(m, np.int32)
    _check(matcher_lib().orbm_distinctive_descriptors(_p(desc), _p(off), m, _p(br), _p(bm), int(device)))
    return br, bm


WORLDPOINT_DTYPE = np.dtype([("valid", "<i4"), ("wx", "<f4"), ("wy", "<f4"), ("wz", "<f4"), ("nx", "<f4"), ("ny", "<f4"),
                             ("nz", "<f4"), ("max_distance", "<f4"), ("min_distance", "<f4"), ("observations", "<i4")])


def predict_scale_thresholds(log_scale_factor, nlevels):
    """orbm_predict_scale_thresholds (host code, no GPU): MapPoint::PredictScale as nlevels-1 float thresholds"""
    t = np.zeros(max(nlevels - 1, 1), np.float32)
    _check(matcher_lib().orbm_predict_scale_thresholds(float(log_scale_factor), int(nlevels), _p(t)))
    return t[:nlevels - 1]


def is_in_frustum(pts, Tcw, cam, geom, viewing_cos_limit, thresholds, nlevels, device=0):
    """orbm_is_in_frustum: Frame::isInFrustum for a list of map points -> MP_DTYPE records"""
    pts = np.ascontiguousarray(pts, WORLDPOINT_DTYPE); T = np.ascontiguousarray(Tcw, np.float32)
    thr = np.ascontiguousarray(thresholds, np.float32)
    out = np.zeros(len(pts), MP_DTYPE)
    _check(matcher_lib().orbm_is_in_frustum(_p(pts), len(pts), _p(T), C.byref(cam), C.byref(geom), float(viewing_cos_limit), _p(thr),
                                    int(nlevels), _p(out), int(device)))
    return out


def search_local_points(kun, desc, uright, geom, sf, pts, mp_desc, Tcw, cam, viewing_cos_limit, thresholds, frame_mp,
                        ext_obs, th, nnratio, device=0):
    """orbm_search_local_points: isInFrustum + SearchByProjection(F, MPs) -> (nmatches, frame_mp', projections)"""
    kun = np.ascontiguousarray(kun, KP_DTYPE); desc = np.ascontiguousarray(desc, np.uint8)
    ur = np.ascontiguousarray(uright, np.float32); sf = np.ascontiguousarray(sf, np.float32)
    pts = np.ascontiguousarray(pts, WORLDPOINT_DTYPE); md = np.ascontiguousarray(mp_desc, np.uint8)
    T = np.ascontiguousarray(Tcw, np.float32); thr = np.ascontiguousarray(thresholds, np.float32)
    fm = np.ascontiguousarray(frame_mp, np.int32).copy()
    eo = None if ext_obs is None else np.ascontiguousarray(ext_obs, np.int32)
    proj = np.zeros(len(pts), MP_DTYPE)
    n = C.c_int(0)
    _check(matcher_lib().orbm_search_local_points(_p(kun), _p(desc), _p(ur), len(kun), C.byref(geom), _p(sf), len(sf), _p(pts), _p(md),
                                          len(pts), _p(T), C.byref(cam), float(viewing_cos_limit), _p(thr), _p(fm), _p(eo),
                                          float(th), float(nnratio), int(device), C.byref(n), _p(proj)))
    return n.value, fm, proj


class Vocabulary:
    """DBoW2 vocabulary on the GPU (orbv_*): from per-node arrays in file order, or from an ORBvoc.txt file."""

    def _ck(self, rc):
        _check(rc, self._L)

    def __init__(self, k=None, L=None, scoring=0, weighting=0, parent=None, is_leaf=None, desc=None, weight=None, path=None,
                 device=0):
        self._L = lib()
        h = C.c_void_p()
        if path is not None:
            self._ck(self._L.orbv_load_text(str(path).encode(), int(device), C.byref(h)))
        else:
            parent = np.ascontiguousarray(parent, np.int32); is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
            desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32); weight = np.ascontiguousarray(weight, np.float64)
            self._ck(self._L.orbv_create(int(k), int(L), int(scoring), int(weighting), len(parent), _p(parent), _p(is_leaf), _p(desc),
                                       _p(weight), int(device), C.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.orbv_destroy(self._h)
            self._h = None

    def info(self):
        v = [C.c_int(0) for _ in range(6)]
        self._ck(self._L.orbv_info(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("k", "L", "scoring", "weighting", "nnodes", "nwords"), [x.value for x in v]))

    def transform(self, desc, levelsup=4):
        """orbv_transform -> (word_id, node_id, weight) per descriptor"""
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(d)
        w = np.zeros(n, np.int32); nid = np.zeros(n, np.int32); wt = np.zeros(n, np.float64)
        self._ck(self._L.orbv_transform(self._h, _p(d), n, int(levelsup), _p(w), _p(nid), _p(wt)))
        return w, nid, wt


def _bow(words, values):
    w = np.ascontiguousarray(words, np.uint32).reshape(-1); v = np.ascontiguousarray(values, np.float64).reshape(-1)
    if len(w) != len(v):
        raise ValueError("a BoW vector needs as many values as word ids")
    return w, v


def score_l1(words1, values1, words2, values2):
    """orbv_score_l1: ORBVocabulary::score of two BoW vectors (L1Scoring), host code"""
    w1, v1 = _bow(words1, values1); w2, v2 = _bow(words2, values2)
    out = C.c_double(0)
    L = lib()
    _check(L.orbv_score_l1(_p(w1), _p(v1), len(w1), _p(w2), _p(v2), len(w2), C.byref(out)), L)
    return out.value


class KeyFrameDatabase:
    """ORB_SLAM2::KeyFrameDatabase on the GPU (orbv_db_*): keyframes are the caller's ids, BoW vectors (word ids, values) arrays."""

    def _ck(self, rc):
        _check(rc, self._L)

    def __init__(self, nwords, device=0, initial_entries=0):
        self._L = lib()
        h = C.c_void_p()
        self._ck(self._L.orbv_db_create(int(nwords), int(device), int(initial_entries), C.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.orbv_db_destroy(self._h)
            self._h = None

    def add(self, kf_id, words, values):
        w, v = _bow(words, values)
        self._ck(self._L.orbv_db_add(self._h, int(kf_id), _p(w), _p(v), len(w)))

    def erase(self, kf_id):
        self._ck(self._L.orbv_db_erase(self._h, int(kf_id)))

    def clear(self):
        self._ck(self._L.orbv_db_clear(self._h))

    def set_covisible(self, kf_id, ids):
        a = np.ascontiguousarray(ids, np.int32).reshape(-1)
        self._ck(self._L.orbv_db_set_covisible(self._h, int(kf_id), _p(a), len(a)))

    def info(self):
        k, e, p, b = C.c_int(0), C.c_int64(0), C.c_int64(0), C.c_size_t(0)
        self._ck(self._L.orbv_db_info(self._h, C.byref(k), C.byref(e), C.byref(p), C.byref(b)))
        return {"keyframes": k.value, "entries": e.value, "pool_entries": p.value, "device_bytes": b.value}

    def score(self, words, values, kf_ids):
        """orbv_db_score -> float64 score of the query against each listed keyframe"""
        w, v = _bow(words, values)
        ids = np.ascontiguousarray(kf_ids, np.int32).reshape(-1)
        out = np.zeros(len(ids), np.float64)
        self._ck(self._L.orbv_db_score(self._h, _p(w), _p(v), len(w), _p(ids), len(ids), _p(out)))
        return out

    def _detect(self, call, hits):
        cap = hcap = max(16, self.info()["keyframes"])   # candidates and listed keyframes are keyframes of the database
        for attempt in range(4):
            cand = np.zeros(cap, np.int32); h = np.zeros(hcap, DB_HIT_DTYPE) if hits else None
            nc, nh = C.c_int(0), C.c_int(0)
            rc = call(_p(cand), cap, C.byref(nc), _p(h), hcap, C.byref(nh))
            if rc == ORBX_ERR_ARG and (nc.value > cap or nh.value > hcap) and attempt < 3:   # keyframes added by another thread meanwhile
                cap, hcap = max(cap, 2 * nc.value), max(hcap, 2 * nh.value)
                continue
            self._ck(rc)
            break
        return (cand[:nc.value].copy(), h[:nh.value].copy()) if hits else cand[:nc.value].copy()

    def detect_loop_candidates(self, words, values, connected, min_score, hits=False):
        """orbv_db_detect_loop -> candidate ids (and, with hits, the DB_HIT_DTYPE records of the listed keyframes in list order)"""
        w, v = _bow(words, values)
        c = np.ascontiguousarray(sorted(connected) if isinstance(connected, (set, frozenset)) else connected, np.int32).reshape(-1)
        return self._detect(lambda *a: self._L.orbv_db_detect_loop(self._h, _p(w), _p(v), len(w), _p(c), len(c), float(min_score), *a), hits)

    def detect_relocalization_candidates(self, words, values, hits=False):
        """orbv_db_detect_reloc -> candidate ids (and, with hits, the records of the listed keyframes)"""
        w, v = _bow(words, values)
        return self._detect(lambda *a: self._L.orbv_db_detect_reloc(self._h, _p(w), _p(v), len(w), *a), hits)


def search_by_bow(q_desc, q_angle, q_valid, c_desc, c_angle, c_valid, node_qstart, q_items, node_cstart, c_items, max_dist,
                  nnratio, check_orientation=True, device=0):
    """orbm_search_by_bow -> (nmatches, match_q)"""
    qd = np.ascontiguousarray(q_desc, np.uint8); qa = np.ascontiguousarray(q_angle, np.float32)
    qv = np.ascontiguousarray(q_valid, np.uint8)
    cd = np.ascontiguousarray(c_desc, np.uint8); ca = np.ascontiguousarray(c_angle, np.float32)
    cv = None if c_valid is None else np.ascontiguousarray(c_valid, np.uint8)
    nqs = np.ascontiguousarray(node_qstart, np.int32); qi = np.ascontiguousarray(q_items, np.int32)
    ncs = np.ascontiguousarray(node_cstart, np.int32); ci = np.ascontiguousarray(c_items, np.int32)
    mq = np.zeros(len(qa), np.int32)
    n = C.c_int(0)
    _check(lib().orbm_search_by_bow(_p(qd), _p(qa), _p(qv), len(qa), _p(cd), _p(ca), _p(cv), len(ca), _p(nqs), _p(qi), _p(ncs),
                                    _p(ci), len(nqs) - 1, int(max_dist), float(nnratio), int(check_orientation), _p(mq),
                                    C.byref(n), int(device)))
    return n.value, mq


def search_for_triangulation(kp1, q_desc, q_flags, kp2, c_desc, c_flags, node_qstart, q_items, node_cstart, c_items, F12, ex, ey,
                             scale_factors, level_sigma2, max_dist=50, check_orientation=True, device=0):
    """orbm_search_for_triangulation -> (nmatches, match_q)"""
    k1 = np.ascontiguousarray(kp1, KP_DTYPE); k2 = np.ascontiguousarray(kp2, KP_DTYPE)
    qd = np.ascontiguousarray(q_desc, np.uint8); cd = np.ascontiguousarray(c_desc, np.uint8)
    qf = np.ascontiguousarray(q_flags, np.uint8); cf = np.ascontiguousarray(c_flags, np.uint8)
    nqs = np.ascontiguousarray(node_qstart, np.int32); qi = np.ascontiguousarray(q_items, np.int32)
    ncs = np.ascontiguousarray(node_cstart, np.int32); ci = np.ascontiguousarray(c_items, np.int32)
    F = np.ascontiguousarray(F12, np.float32); sf = np.ascontiguousarray(scale_factors, np.float32)
    s2 = np.ascontiguousarray(level_sigma2, np.float32)
    mq = np.zeros(len(k1), np.int32)
    n = C.c_int(0)
    _check(lib().orbm_search_for_triangulation(_p(k1), _p(qd), _p(qf), len(k1), _p(k2), _p(cd), _p(cf), len(k2), _p(nqs), _p(qi),
                                               _p(ncs), _p(ci), len(nqs) - 1, _p(F), float(ex), float(ey), _p(sf), _p(s2), len(sf),
                                               int(max_dist), int(check_orientation), _p(mq), C.byref(n), int(device)))
    return n.value, mq
