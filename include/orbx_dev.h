/* orbx_dev.h - test hooks of the DEVELOPER build of the library (orb_slam2v2-1_amd/lib/liborbx_hip_dev.so, built with
 * -DORBX_DEVELOPER from the same sources as the product library).  The product library liborbx_hip.so exports none of these:
 * `nm -D liborbx_hip.so | grep -c debug` is 0.  The hooks are read-only views of intermediate results (SURVEY.md section 8 rows that
 * have no output of their own); the staged parity tests load the developer build for them, everything timed or end-to-end loads
 * the product library.  Results of the two builds are identical.
 * The developer build also accepts the option keys 0, 1 and 7 of orbx_set_option (stop a kernel after phase n: outputs incomplete;
 * 7 = 8 / 9: k_octree_pyr leaves time stamps instead of the 0 / 1 fall-back flag in the record orbx_debug_octree_fallbacks reads -
 * only then; with the key at 0 the record is the product build's). */
#ifndef ORBX_DEV_H
#define ORBX_DEV_H
#include "orbx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Stage introspection for parity tests (not part of the reference API):
 * stage 0 = FAST candidates before the quad-tree (vToDistributeKeys order),
 * stage 1 = keypoints kept by DistributeOctTree (list order).
 * out: triples (x, y, score) int32, coordinates relative to minBorder (16,16). */
int orbx_debug_level_points(orbx_extractor_t *h, int b, int level, int stage, int32_t *out_xys, int cap,
                            int *n_out);

/* Test hooks for two rows of the scope table that have no output of their own.
 * orbx_debug_blur_patches (a8, cv::GaussianBlur 7x7 sigma 2 - fused into the descriptor kernel, never stored): enable = 1, then
 * orbx_extract of ONE image with cap <= the handle's keypoint bound, then out != NULL fetches the 37x37 blurred block around each
 * of the first n keypoints (n * 1369 bytes, keypoint order); enable = 0 releases the buffer.
 * orbm_debug_features_in_area (a12, Frame::GetFeaturesInArea src/Frame.cc:342-395): the indices the query returns, in the
 * reference's order (column-major over grid cells, insertion order inside a cell) - the order every matcher's "first minimum
 * wins" depends on. */
int orbx_debug_blur_patches(orbx_extractor_t *h, int enable, uint8_t *out, int n);
/* Probe hook: out[b * nlevels + l] = 1 iff the quad-tree of level l of image b of the last call was redone by the exact form
 * (k_octree_pyr's count pyramid too shallow for it; results are the same, the level just took longer).  n <= B * nlevels. */
int orbx_debug_octree_fallbacks(orbx_extractor_t *h, int32_t *out, int n);
/* a8, the other form: levels whose keypoint budget makes per-keypoint blurring the more expensive way are blurred as a whole by
 * k_blur_levels and the descriptor kernel only gathers (src/ORBextractor.cc:1083-1090 does exactly this for every level).
 * *mask_out (may be NULL) = levels of the last call that took this form (bit l); dst != NULL fetches level `level` of image b
 * (inner ROI, dst_stride bytes per row) - ORBX_ERR_ARG when that level is not in the mask.  ORBX_OPT_BLUR_FORM (orbx_set_option):
 * 1 = no level, 2 = every level; ORBX_OPT_BLUR_THRESHOLD = the rule's threshold in percent (level-wide iff nfeatures_l * 37^2 * 100 >=
 * thr * w_l * h_l).  Results never depend on the form. */
int orbx_debug_blurred_level(orbx_extractor_t *h, int b, int level, uint8_t *dst, int dst_stride, unsigned *mask_out);
int orbm_debug_features_in_area(const orbx_keypoint_t *kun, int n, const orbm_grid_geom_t *g, float x, float y, float r,
                                int min_level, int max_level, int32_t *out_idx, int *n_out, int device);
/* Test hook: the device's restatement of libm cosf / sinf (the float overloads src/ORBextractor.cc:113 resolves to) on n
 * host angles in [0, 2 pi]; the descriptor kernel uses exactly this routine. */
int orbx_debug_sincosf(const float *angles, int n, float *sin_out, float *cos_out, int device);

/* Which code the matchers of the calling host thread ran (the size thresholds of the guided searches and of the stereo matcher pick
 * different kernels, LDS plans and fall-backs; the results never depend on the choice, so only these hooks can tell them apart).
 * orbm_debug_match_path: the last guided search of this thread (orbm_search_for_initialization, orbm_search_by_projection_mp / _frame
 * (+ _device), orbm_search_local_points (+ _device), orbm_match_windows): out[0] = the resolver that produced the result
 * (ORBM_PATH_RES_*), out[1] = why the fast path fell back to the exact kernels (ORBM_PATH_FB_*), out[2] = the dynamic LDS bytes the
 * fast path's resolver requested (0: it launched none).  A call that returned before any kernel (no queries, no keypoints, an
 * argument error) leaves RES_NONE. */
#define ORBM_PATH_RES_NONE 0
#define ORBM_PATH_RES_PAR_Q2 1   /* k_resolve_par, 2 queries per thread (m <= 2048) */
#define ORBM_PATH_RES_PAR_Q4 2   /* k_resolve_par, 4 queries per thread (2048 < m <= 4096) */
#define ORBM_PATH_RES_WAVE 3     /* the single-wave speculative resolvers (k_resolve_mp / _frame / _windows / _init) */
#define ORBM_PATH_RES_EXACT 4    /* the exact one-workgroup kernels */
#define ORBM_PATH_FB_NONE 0
#define ORBM_PATH_FB_N 1         /* n > 30000 keypoints */
#define ORBM_PATH_FB_INIT_SIZE 2 /* SearchForInitialization: n2 > 7000 or n1 > 65535 (LDS plan of k_resolve_init) */
#define ORBM_PATH_FB_CAND_CAP 3  /* a query had more than CAND_CAP (512) candidates */
#define ORBM_PATH_FB_QK 4        /* a query ran out of its QK (8) kept candidates */
#define ORBM_PATH_FB_LDS 5       /* hipFuncSetAttribute or the launch of k_resolve_par was refused */
#define ORBM_PATH_FB_OPTION 6    /* ORBM_OPT_EXACT_KERNELS */
int orbm_debug_match_path(int64_t *out);
/* The plan of the fast path, launching nothing: mode 0 = SearchByProjection(F, MPs), 1 = SearchByProjection(cur, last), 2 = projected
 * windows, 3 = SearchForInitialization (m = n1, n = n2); for the thread's resolver option and the device.  out[0] = ORBM_PATH_RES_*
 * (EXACT: the fast path falls back before its resolver), out[1] = the resolver's dynamic LDS bytes, out[2] = the static LDS of that
 * kernel instance (hipFuncGetAttributes), out[3] = the device's LDS limit per workgroup. */
int orbm_debug_resolve_plan(int mode, int m, int n, int device, int64_t *out);
/* The last stereo matcher call of this thread (orbm_stereo, orbm_stereo_batch_device(_prev), orbx_stereo_frame(_view)):
 * out[0] = the median / finish step kept the SAD values in LDS (cap <= SM_LDS_CAP), out[1] = bhShift, out[2] = nbins (row bins of
 * level 0), out[3] = 1 iff a left keypoint of that call had more than ST_CAND candidates and restarted its list. */
int orbm_debug_stereo_path(int32_t *out);

/* The launch rule of an extraction call (csrc/orbx_plan.h: plan_chunk), by itself: no HIP call, no handle, works without a GPU.
 * in = PlanInput, out = ChunkPlan, as flat int32 arrays in the structs' field order:
 *   in  (ORBX_DEBUG_PLAN_INPUT_INTS):  B, nl, totalStrips, stripLevels, octBigMask, lastChunks, prof, profFast, skipPyr, pfUsed,
 *        evPyrDone, dbgBlur, sliceScratch, fastTileStride, fastScoreStride, sparseRecent, ncells[16], opt[32]
 *   out (ORBX_DEBUG_CHUNK_PLAN_INTS):  usePyr, strips, stripLevels, fastCells, es, histOct, multiWg, fused, gather, bigMask, wideOct,
 *        compact, sparseForm, sparsePerCell, rowFlags, sparseHint (0 nobody, 1 k_octree_pyr, 2 k_gather), earlyLv, aSplit,
 *        octForm (0 exact alone, 1 big = multi-workgroup, 2 early, 3 split, 4 single), sweepSlices, sweepShared, orderKernel,
 *        fastDoneAt (-1 never, 0 behind FAST, 1 behind the quad-tree, 2 behind the descriptors, 3 together with FAST), fastPhase, octPhase,
 *        octStop, descLdsPad (bytes), nslice[16]
 * n_in / n_out must be exactly those counts.  ORBX_ERR_UNSUPPORTED (and the invariant's text in orbx_last_error) when the plan breaks a
 * constraint the kernels rely on - launch_chunk then launches nothing.
 * orbx_debug_last_plan: the ChunkPlan that chunk 0 of the handle's last extraction call executed (a copy kept in the handle). */
#define ORBX_DEBUG_PLAN_INPUT_INTS 64
#define ORBX_DEBUG_CHUNK_PLAN_INTS 43
int orbx_debug_plan_chunk(const int32_t *in, int n_in, int32_t *out, int n_out);
int orbx_debug_last_plan(const orbx_extractor_t *h, int32_t *out, int n_out);

/* What an image size decides for an extractor (csrc/orbx_size_plan.h: extractor_tables + plan_size), by itself: no HIP call, no handle,
 * works without a GPU.  Arguments as orbx_create takes them, the image size, and ORBX_OPT_PYRAMID_TILE (0 = default).
 *   tables      [4][16] float: sf | isf | sig2 | isig2 (written for every legal extractor, also when the size is refused)
 *   nfeat_umax  [32] int32: features per level [16] | umax [16]
 *   geom        LevelGeom[16] as bytes (geom_bytes must be their exact size, 16 * 144)
 *   tab         the first min(tab_cap, tabWords) table words (tab_cap = 0: none; call again with the tabWords of scalars)
 *   scalars     (ORBX_DEBUG_SIZE_PLAN_INTS int64): max_kp, totalCells, maxNodeCap, lvlKpCap, pyrImgBytes, slotsPerImg, keysPerImg, fastTileStride,
 *        fastScoreStride, fastTileRows, fastLdsPerWave, totalStrips, stripLevels, octLdsBytes, octPyrLdsBytes, octPyrWords, octBigMask, octDeepMax,
 *        octSliceStride, histStride, pyrTilesX, pyrTilesY, pyrXSpanOff, pyrYSpanOff, pyrBufBytes, pyrMaxDim, pyrMaxPar, pyrLdsBytes, nChains[0],
 *        nChains[1], tabWords, stripBase[17], chains[2][8] as 8 ints each (la, lb, tilesX, tilesY, xSpanOff, ySpanOff, bufBytes, maxRows)
 * Returns what ensure_plan would for that size: ORBX_OK, or ORBX_ERR_ARG / ORBX_ERR_UNSUPPORTED with the reason in orbx_last_error (geom, tab and
 * scalars are then not written). */
#define ORBX_DEBUG_SIZE_PLAN_INTS 176
int orbx_debug_size_plan(int nfeatures, float scale_factor, int nlevels, int w, int h, int pyr_tile, float *tables, int32_t *nfeat_umax,
                         uint8_t *geom, int geom_bytes, int32_t *tab, int tab_cap, int64_t *scalars, int n_scalars);

/* The records k_pyr_level's waves read (csrc/orbx_size_plan.h: plan_pyr_records) have a hook of their own, declared in orbx_dev_pyr.h. */

/* The per-thread scratch of the matchers as the CALLING host thread holds it, read only: no HIP call,
 * nothing allocated, works without a GPU and on a thread that never called a matcher (capacities 0, devices -1).
 *   out (ORBM_DEBUG_THREAD_SCRATCH_INTS): arena capacity in bytes, arena device (-1: none), arena call counter, 1 / 0 the arena has a
 *        stream, 1 / 0 the arena has a completion word, staging-pair capacity, staging-pair device, BoW scratch capacity, BoW scratch
 *        device
 * n_out must be exactly that count.  The arena serves the fast path of the guided searches, the staging pair the exact kernels of the
 * host-array entry points, the BoW scratch orbv_transform / orbm_search_by_bow / orbm_search_for_triangulation; capacities only grow
 * until orbx_thread_release_scratch() returns all three to 0 / -1 (the call counter stays). */
#define ORBM_DEBUG_THREAD_SCRATCH_INTS 9
int orbm_debug_thread_scratch(int64_t *out, int n_out);

/* Fill fresh scratch.  Every scratch block of the library - device (hipMalloc) and pinned (hipHostMalloc): the extractor's plan buffers,
 * staging and frame records, the matchers' arena and its mirror, the staging pairs, the BoW scratch, the keyframe database, the cloud /
 * octree / rgbd / rectify / stereo scratch - is allocated through one wrapper pair (csrc/orbx_internal.h).  With enable != 0 the wrapper
 * fills a NEW block with the 32-bit `word` before anything else happens to it: a device block by a 32-bit memset that has completed when
 * the wrapper returns, a pinned block by a host loop (bytes behind the last whole word repeat the word's bytes, little endian).  The
 * explicit initialisations (the zeroed plan buffers, the completion words, the frame records' memset) follow the fill as they follow
 * the allocation.  No result may depend on the word: a recycled block holds whatever its last owner left, a first block usually zero
 * pages, and tests/test_scratch_fill_gpu.py runs every module on blocks filled with 1 and with 3.  Scratch is made fresh by
 * orbx_thread_release_scratch() or a new handle; there is no hook that refills memory between calls.
 * The state is process-wide and atomic, off by default; a set (either value of enable) restarts the statistics.
 * orbx_debug_alloc_fill_stats: out[0] = blocks filled, out[1] = bytes filled since the last set.  Neither makes a HIP call. */
int orbx_debug_set_alloc_fill(int enable, uint32_t word);
int orbx_debug_alloc_fill_stats(int64_t out[2]);

/* Stream order under injected stalls (tests/stream_stall.py, tests/test_stream_order_gpu.py).
 * orbx_debug_stall_stream: one wave of k_spin on `stream` (NULL = the default stream) of `device` - the bounded loop on the 100 MHz wall
 * clock orbx_side_stream_for probes queues with - for `microseconds` in [1, 50000] (anything else: ORBX_ERR_ARG).  It launches nothing
 * else and waits for nothing: what is queued on the stream afterwards starts that much later, and a consumer on another stream that
 * lacks its wait reads what the buffers held before.
 * orbx_debug_streams: out[0..2] = the handle's own stream, side[0], side[1] (NULL when h is NULL), out[3] = the calling thread's matcher
 * arena stream, out[4] = its matcher staging-pair stream (NULL: the thread holds none).  n_out must be exactly 5.  Read only, no HIP call. */
int orbx_debug_stall_stream(void *stream, int microseconds, int device);
int orbx_debug_streams(orbx_extractor_t *h, void **out, int n_out);

#ifdef __cplusplus
}
#endif
/* Which input form an extraction call ran - level 0 read in place or copied - is declared in orbx_dev_level0.h, which comes with this header. */
#include "orbx_dev_level0.h"
#endif
