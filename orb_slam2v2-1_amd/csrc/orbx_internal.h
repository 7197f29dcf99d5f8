// orbx_internal.h — shared declarations of the HIP implementation (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "orbx.h"
#include "orbx_size_plan.h"   // LevelGeom / ChainPlan / ExtractorTables / SizePlan / plan_size: what an image size decides; the limits and reference constants

// the Gaussian's Q8 taps k3 | k2 << 8 | k1 << 16 | k0 << 24 of every flavour but ORBX_GAUSS_FIXED_TAPS: cvRound(256 g_i) = 18 34 49 55 (sum 257)
#define ORBX_GAUSS_TAPS_DEFAULT (18u | (34u << 8) | (49u << 16) | (55u << 24))
#define ORBX_DESC_R 18      // max |rotated tap| : pattern radius^2 = 338 -> cvRound <= 18
#define ORBX_EV_RING 32
#define ORBX_MAX_CHUNKS 4      // chunks a batch may be cut into (launch_pipeline)
#define ORBX_SIDE_STREAMS 2    // handle-owned streams for the chunks behind the first
#define ORBX_HIST_IMAGES 4     // batches up to this size: the FAST stage histograms its emissions for the quad-tree (FastHist)

#include "orbx_plan.h"   // PlanInput / ChunkPlan / plan_chunk / chunk_count: the launch rule of an extraction call

#define ORBX_HIP(call)                                                                      \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            orbx_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                           __LINE__);                                                       \
            return (e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice ||                \
                    e_ == hipErrorNoBinaryForGpu || e_ == hipErrorInsufficientDriver)       \
                       ? ORBX_ERR_NO_DEVICE                                                 \
                       : ORBX_ERR_HIP;                                                      \
        }                                                                                   \
    } while (0)

// Every scratch allocation of the library (device and pinned) goes through this pair.  The product build's is the plain call.  The
// developer build's can fill a new block with one 32-bit word before anyone else sees it (orbx_debug_set_alloc_fill, include/orbx_dev.h;
// off by default), so that a test runs every call on scratch that holds neither zero pages nor its own earlier results
// (tests/test_scratch_fill_gpu.py).  A device block's fill has completed when the wrapper returns.
#ifdef ORBX_DEVELOPER
hipError_t orbx_internal_scratch_filled(void *p, size_t bytes, bool pinned);   // orbx_extract.hip
template <class T> static inline hipError_t scratch_malloc(T **p, size_t bytes) {
    const hipError_t e = hipMalloc((void **)p, bytes);
    return e != hipSuccess ? e : orbx_internal_scratch_filled((void *)*p, bytes, false);
}
template <class T> static inline hipError_t scratch_host_malloc(T **p, size_t bytes, unsigned flags) {
    const hipError_t e = hipHostMalloc((void **)p, bytes, flags);
    return e != hipSuccess ? e : orbx_internal_scratch_filled((void *)*p, bytes, true);
}
#else
template <class T> static inline hipError_t scratch_malloc(T **p, size_t bytes) { return hipMalloc((void **)p, bytes); }
template <class T> static inline hipError_t scratch_host_malloc(T **p, size_t bytes, unsigned flags) { return hipHostMalloc((void **)p, bytes, flags); }
#endif

// Level 0 of a batch read IN PLACE from the caller's images (orbx_extract_batch_device_padded): image b's padded level 0 - the layout
// of orbx_level0_layout, which is LevelGeom[0]'s - starts at base + b * imgBytes.  base == NULL: level 0 is in the pyramid block like
// every other level (k_pyr_pad<true> copied it there).  A kernel argument of everything that addresses level 0 (level_base,
// orbx_extract_dev.h), and a property of each pyramid buffer of the handle: it travels with the buffer when they rotate.
struct Level0 { const uint8_t *base; size_t imgBytes; };
// Where level l of image b starts.  Image and level are wave-uniform at every call site, so the choice is one select on the scalar
// unit; levels >= 1 always live in the pyramid block.
__device__ __forceinline__ const uint8_t *level_base(const uint8_t *pyr, size_t pyrImgBytes, const Level0 &z, int b, int l, unsigned long long poff) {
    const bool ext = l == 0 && z.base != nullptr;
    const uint8_t *base = ext ? z.base : pyr;
    const size_t img = ext ? z.imgBytes : pyrImgBytes, off = ext ? 0 : (size_t)poff;
    return base + (size_t)b * img + off;
}

struct orbx_extractor {
    int nfeatures, nlevels, ini_th, min_th, device;
    double scale_factor;
    ExtractorTables tb;              // scale, sigma, features per level, umax (extractor_tables)
    orbx_flavour_t flavour;          // which OpenCV build the handle stands in for (orbx_create_flavoured); fixed for the handle's life
    int opt[ORBX_NUM_OPTIONS];       // per-handle options (orbx_set_option): alternative kernels / arrangements with identical results

    // plan (depends on image size / batch capacity)
    int pw, ph, pB;  // planned image size and batch capacity (0 = none)
    SizePlan sp;     // everything the image size decides (plan_size); ensure_plan reads the size nowhere else
    int32_t *d_octFallback;
    // multi-workgroup quad-tree of large levels: scratch (sized for every level so that a developer knob can force it)
    uint32_t *d_octPart, *d_octLeaf, *d_octBest; int32_t *d_octState;
    // device buffers
    LevelGeom *d_geom;
    int32_t *d_tab;
    PyrRecords pr;       // k_pyr_level's column and band records of the planned size (plan_pyr_records), uploaded with geom and tab
    PyrColRec *d_pyrCols; uint32_t *d_pyrBands;
    uint8_t *d_pyr;
    uint32_t *d_cellCnt, *d_cellRaw, *d_slots, *d_cand, *d_lvlKp;
    uint16_t *d_nodeOf;
    int32_t *d_candCnt, *d_lvlCnt;
    int candStale;       // > 0: the compacted key arrays (d_cand / d_candCnt of every level) of that many images were not written by the last call
                         // (k_octree_pyr read the cell lists in place); k_gather materialises them on demand (test hooks)
    int32_t *h_sparseSeen, *d_sparseSeen; int callSeq;   // host-mapped word: sequence number of the last call that flagged a corner-sparse level
    uint32_t *d_octPartBest, *d_octPartCnt; int32_t *d_octSliceState;   // shared sweeps of large levels in a batch (OctSrc::nslice)
    uint32_t *d_histCnt, *d_histBest;   // [ORBX_HIST_IMAGES][nlevels][histStride] deepest-depth histogram of small batches (FastHist)
    int32_t *d_sparse;   // [B][nlevels] verdict of the last call: level with few FAST candidates (k_gather writes, k_fast_strips of the next call reads)
    // staging for the host API
    uint8_t *d_in; size_t d_in_bytes;
    orbx_keypoint_t *d_kps; uint8_t *d_desc; int32_t *d_counts; int out_cap, out_B;
    orbx_keypoint_t *h_kps; uint8_t *h_desc; int32_t *h_counts;   // pinned mirrors of the three above
    float *d_sfr; float *h_sfr; int sfr_cap;   // orbx_stereo_frame: mvuRight | mvDepth | nmatch of one frame (device + pinned mirror)
    // orbx_stereo_frame_view: two alternating frame records (HBM + pinned host twin, and the twin as kernels address it), pinned staging for pageable images
    uint8_t *fv_d[2], *fv_h[2], *fv_hdev[2]; int fv_cap, fv_next;
    uint8_t *fv_stage, *fv_stage_dev; size_t fv_stage_bytes;
    int32_t *fv_flag, *fv_flag_dev; int fv_seq;   // completion word of a latency call (coherent pinned memory): its last kernel stores the call's number, the host polls it
    long long descHostDelta;   // != 0 while a latency call is being issued: k_describe repeats its stores at address + delta (the record's pinned twin)
    uint8_t *d_dbgBlur; int dbgBlurCap;   // test hook: blurred 37x37 blocks of a single-image call (orbx_debug_blur_patches)
    hipStream_t stream;      // own stream
    hipStream_t side[ORBX_SIDE_STREAMS]; hipEvent_t evPyr[ORBX_MAX_CHUNKS], evJoin[ORBX_SIDE_STREAMS]; int lastChunks;   // chunk overlap (launch_pipeline)
    // pyramid of the NEXT batch, built ahead on side[0] into a second buffer (orbx_extract_batch_device_prefetch)
    uint8_t *d_pyrAlt; size_t pyrAltBytes; int pfValid, pfUsed, pfB, pfW, pfH, pfStride; const uint8_t *pfImgs; size_t pfImgStride;
    // levels blurred as a whole (k_blur_levels) for k_describe's gather form: buffers with the pyramid's geometry, swapped with it
    uint8_t *d_blur, *d_blurAlt; size_t blurBytes, blurAltBytes; unsigned blurMaskLast, blurMaskAlt;
    // split call (launch_chunk): records of the small levels described ahead, and the events between the two streams
    orbx_keypoint_t *d_kpsB; uint8_t *d_descB; size_t splitBytes; hipEvent_t evGather, evOctA;
    uint8_t *d_pyrNext; size_t pyrNextBytes; int pyrBuffers;   // three-buffer mode (orbx_set_pyramid_buffers): the pyramid built ahead gets a buffer of its own, the previous one survives it
    int prevPyrValid;   // d_pyrAlt still holds the pyramid of the call before the last one (orbm_stereo_batch_device_prev)
    Level0 lv0, lv0Alt, lv0Next;   // where level 0 of d_pyr / d_pyrAlt / d_pyrNext lives (base NULL: in the buffer itself); swapped with the buffers
    int lv0Stale;       // > 0: level 0 of that many images of d_pyr has not been copied from lv0 (test hooks copy it on demand, ensure_level0)
    int pfPadded;       // the pyramid built ahead was asked for through the in-place entry point (part of what the next call must repeat)
    hipEvent_t evFastDone, evPrefetch;
    hipStream_t last_stream; // stream of the last batch call (NULL is a stream too: the HIP default stream)
    int last_valid;          // ... once there has been one
    int lastB;
    ChunkPlan lastPlan;      // the plan chunk 0 of the last call executed (orbx_debug_last_plan)
    int framesStale;         // > 0: the frames of levels >= 1 of that many images have not been written (see ensure_frames)
    // scratch of Frame::ComputeStereoMatches when this handle is the LEFT extractor (orbx_match.hip: stereo_scratch_reserve)
    int32_t *st_sad; uint2 *st_rc; int32_t *st_binStart; uint4 *st_items; size_t st_n; int st_nB;
    hipStream_t st_stream;   // stream of the last stereo call on this handle
    // per-stage HIP-event timing: a ring of event sets so that timing never forces a sync
    int profiling; unsigned prof_calls;
    hipEvent_t ev[ORBX_EV_RING][ORBX_NUM_STAGES];
    unsigned char ev_pending[ORBX_EV_RING];
    int ev_head;
    double acc_ms[ORBX_NUM_STAGES];
    long acc_n;
    struct RgbdScratch *rgbd;   // orbx_rgbd_frame: colour / gray / depth images and the frame's results (orbx_rgbd.hip), NULL until first used
    struct RectScratch *rect;   // orbx_stereo_frame(_view)_rectified: raw pair, its pinned staging, rectified gray pair (orbx_rectify.hip), NULL until first used
};

// extractor internals used by the matcher side
void orbx_internal_free_stereo_scratch(orbx_extractor *h);   // orbx_match.hip
void orbx_internal_free_rgbd_scratch(orbx_extractor *h);     // orbx_rgbd.hip
void orbx_internal_free_rect_scratch(orbx_extractor *h);     // orbx_rectify.hip
// orbx_stereo_frame on a pair already in HBM on the handle's device (image 1 at d_pair + img_bytes), queued on the handle's stream (orbx_extract.hip)
int orbx_internal_stereo_frame_device(orbx_extractor *h, const uint8_t *d_pair, int w, int hgt, int stride, size_t img_bytes, float mbf,
                                      float mb, int cap, orbx_keypoint_t *kl, uint8_t *dl, int *nl, orbx_keypoint_t *kr, uint8_t *dr,
                                      int *nr, float *uright, float *depth, int *nmatch);
// ComputeStereoMatches of the frame in image slots 0 / 1 of h with the record layout of orbx_stereo_frame_view (orbx_match.hip)
int orbx_internal_stereo_frame_record(orbx_extractor *h, uint8_t *d_rec, uint8_t *rec_hostdev, int cap, float mbf, float mb, hipStream_t st, bool recordsOnHost,
                                      int32_t *doneFlag, int doneSeq, int *flagArmed);
void orbx_internal_release_match_scratch();                  // orbx_match.hip       (thread-local StagePair, orbx_stage.h)
void orbx_internal_release_arena();                          // orbx_match_fast.hip  (thread-local arena)
void orbx_internal_release_bow_scratch();                    // orbx_bow.hip         (thread-local scratch)
void orbx_internal_release_pose_scratch();                   // orbx_poseopt.hip     (thread-local StagePair)
void orbx_internal_release_init_scratch();                   // orbx_initializer.hip (thread-local StagePair)
void orbx_internal_release_sim3_scratch();                   // orbx_sim3.hip        (thread-local StagePair)
void orbx_internal_release_pnp_scratch();                    // orbx_pnp.hip         (thread-local StagePair)
void orbx_internal_release_sim3opt_scratch();                // orbx_sim3opt.hip     (thread-local StagePair)
void orbx_internal_release_newpoints_scratch();              // orbx_newpoints.hip   (thread-local StagePair)
void orbx_internal_release_lba_scratch();                    // orbx_lba.hip         (thread-local StagePair)
void orbx_internal_release_essential_scratch();              // orbx_essential.hip   (thread-local StagePair)
void orbx_internal_release_covis_scratch();                  // orbx_covis.hip       (thread-local StagePair)
void orbx_internal_release_mapcorrect_scratch();             // orbx_mapcorrect.hip  (thread-local StagePair)
// orbx_covis.hip: the host checks of an observation table and of a query set (ORBX_ERR_ARG with a message), for orbx_localmap.hip too
int orbx_internal_cov_check_table(const char *fn, const orbc_table_t *t);
int orbx_internal_cov_check_queries(const char *fn, const orbc_table_t *t, const orbc_queries_t *q, bool distinct);
// orbx_bow.hip: ORBmatcher::SearchForTriangulation's node-list checks and its launch sequence on device-resident arrays, for its own
// entry point and for orbl_create_new_map_points (orbx_newpoints.hip)
int orbx_internal_tri_check(const char *fn, const int32_t *node_qstart, const int32_t *q_items, int nq, const int32_t *node_cstart,
                            const int32_t *c_items, int nc, int nnodes);
void orbx_internal_tri_launch(const orbx_keypoint_t *d_k1, const uint8_t *d_qd, const uint8_t *d_qf, float *d_qa, int nq, const orbx_keypoint_t *d_k2,
                              const uint8_t *d_cd, const uint8_t *d_cf, float *d_ca, int nc, const int32_t *d_nqs, const int32_t *d_qi,
                              const int32_t *d_ncs, const int32_t *d_ci, int nnodes, const float *F12_9, float ex, float ey,
                              const float *scale_factors, const float *level_sigma2, int nlevels, int max_dist, int check_orientation,
                              int32_t *d_match_q, int32_t *d_out2, hipStream_t st);
#ifdef ORBX_DEVELOPER
// what the calling thread holds of each of the three, for orbm_debug_thread_scratch (include/orbx_dev.h): no HIP call, nothing allocated
void orbx_internal_arena_info(int64_t *out5);                // capacity, device, call counter, has a stream, has a completion word
void orbx_internal_match_scratch_info(int64_t *out2);        // capacity, device
void orbx_internal_bow_scratch_info(int64_t *out2);          // capacity, device
// the calling thread's arena stream / staging-pair stream (NULL: it holds none), for orbx_debug_streams
void *orbx_internal_arena_stream();                          // orbx_match_fast.hip
void *orbx_internal_match_scratch_stream();                  // orbx_match.hip
#endif
// the address a kernel reads an image at (device, pinned or managed memory), or NULL for ordinary pageable host memory (orbx_extract.hip)
const uint8_t *orbx_internal_device_visible(const uint8_t *p);
int orbx_internal_level(const orbx_extractor *h, int level, int *w, int *hgt, int *pstride,
                        unsigned long long *poff);

// orbx_match_fast.hip: parallel candidate search + speculative resolution.  Return ORBX_OK
// (results written), 1 (= fall back to the exact one-workgroup kernel) or a negative error.
int fast_search_for_initialization(const orbx_keypoint_t *k1, const uint8_t *d1, int n1, const orbx_keypoint_t *k2,
                                   const uint8_t *d2, int n2, const orbm_grid_geom_t *g2, float *prev, int32_t *m12,
                                   int window, float nnratio, int check_ori, int device, int *nmatches);
// frame arrays that are already device-resident (the *_device matcher entry points): the kernels then run on `stream`
struct DevFrame { hipStream_t stream; };
struct FrustumArgs { const orbm_worldpoint_t *pts; const float *Tcw16; const orbm_camera_t *cam; float viewCosLimit; const float *thr; };
int fast_search_by_projection_mp(const orbx_keypoint_t *kun, const uint8_t *desc, const float *uright, int n,
                                 const orbm_grid_geom_t *g, const float *sf, int nlevels, const orbm_mappoint_t *mps,
                                 const uint8_t *mp_desc, int m, int32_t *frame_mp, const int32_t *ext_obs, float th,
                                 float nnratio, int device, int *nmatches, const FrustumArgs *world = nullptr,
                                 orbm_mappoint_t *proj_out = nullptr, const DevFrame *dev = nullptr);
int fast_is_in_frustum(const orbm_worldpoint_t *pts, int m, const float *Tcw16, const orbm_camera_t *cam,
                       const orbm_grid_geom_t *g, float viewCosLimit, const float *thr, int nlevels, orbm_mappoint_t *out,
                       int device);
int fast_search_by_projection_frame(const orbx_keypoint_t *kun, const uint8_t *desc, const float *uright, int n,
                                    const orbm_grid_geom_t *g, const float *sf, int nlevels, const orbm_camera_t *cam,
                                    const float *Tc16, const float *Tl16, const orbm_lastpoint_t *last,
                                    const uint8_t *last_desc, int nlast, int32_t *cur_mp, const int32_t *ext_obs,
                                    float th, int mono, int check_ori, int device, int *nmatches, const DevFrame *dev = nullptr);
int fast_match_windows(const orbx_keypoint_t *kun, const uint8_t *desc, const float *uright, int n,
                       const orbm_grid_geom_t *g, const orbm_grid_geom_t *ga, const orbm_window_query_t *q,
                       const uint8_t *qdesc, int m,
                       int32_t *holder, const int32_t *ext_blocks, int max_dist, int check_ori, int device, int *nmatches);
int fast_best_in_windows(const orbx_keypoint_t *kun, const uint8_t *desc, const float *uright, int n,
                         const orbm_grid_geom_t *g, const orbm_grid_geom_t *ga, const orbm_window_query_t *q,
                         const uint8_t *qdesc, int m, const float *inv_sigma2, int nlevels, int32_t *best_idx,
                         int32_t *best_dist, int device);
int fast_distinctive_descriptors(const uint8_t *desc, const int32_t *offsets, int npoints, int32_t *best_row,
                                 int32_t *best_median, int device);
extern thread_local int t_matchExact;   // orbm_set_thread_option(ORBM_OPT_EXACT_KERNELS): this thread's guided searches take the exact one-workgroup kernels
// What the last guided search / stereo call of this host thread ran (codes: ORBM_PATH_* of include/orbx_dev.h); written by both builds,
// read by the developer build's orbm_debug_match_path / orbm_debug_stereo_path
struct MatchPath { int resolver, fallback; long long lds; };
struct StereoPath { int useLds, bhShift, nbins, device; };
extern thread_local MatchPath t_matchPath;
extern thread_local StereoPath t_stereoPath;

// XCD-aware block -> (image, block-in-image) map for grids of (blocks per image, images).  Workgroups are dealt round-robin
// to the 8 XCDs in linear-id order and every XCD has its own L2, so with the identity map neighbouring blocks - which
// share 128-byte lines of the same pyramid rows - land in different L2s and each line crosses the fabric several times
// (measured on k_fast_cells: FETCH_SIZE 2.0x the algorithmic bytes).  With this map XCD x works through a contiguous
// eighth of the (image, block) list, i.e. whole images.  A bijection for any grid size.
__device__ __forceinline__ void xcd_block_map(int &bx, int &b) {
    const unsigned nbx = gridDim.x, total = nbx * gridDim.y, lin = blockIdx.y * nbx + blockIdx.x;
    const unsigned xcd = lin & 7u, idx = lin >> 3, q = total >> 3, r = total & 7u;
    const unsigned pos = xcd * q + min(xcd, r) + idx;   // XCD x owns q (+1 if x < r) consecutive positions
    // the division runs on the vector ALU (no scalar float unit): hand the (uniform) results back to scalar registers so that
    // everything derived from them - image base pointers above all - stays scalar
    b = __builtin_amdgcn_readfirstlane((int)(pos / nbx));
    bx = __builtin_amdgcn_readfirstlane((int)(pos - (unsigned)b * nbx));
}
