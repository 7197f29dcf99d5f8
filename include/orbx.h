/*
 * orbx.h — C ABI of the MI355X-native ORB front-end + Hamming matchers.
 *
 * This is the drop-in boundary for ONE hot path of kimwin2/ORB_SLAM2v2-1:
 *   ORBextractor::operator()            reference: src/ORBextractor.cc:1043-1105
 *   Frame::ComputeStereoMatches         reference: src/Frame.cc:481-655
 *   ORBmatcher::SearchForInitialization reference: src/ORBmatcher.cc:405-520
 *   ORBmatcher::SearchByProjection x2   reference: src/ORBmatcher.cc:45-129, 1330-1472
 *   ORBmatcher::DescriptorDistance      reference: src/ORBmatcher.cc:1649-1665
 * Plain pointers and sizes only; POD structs; the caller allocates every output.
 * All functions return 0 on success or a negative orbx_status; nothing throws.
 * The implementation is HIP for gfx950 only — there is NO CPU fallback: every entry
 * point that needs the GPU fails with ORBX_ERR_NO_DEVICE when none is usable.
 *
 * Pointers named d_* are DEVICE pointers (e.g. torch tensor .data_ptr()); `stream`
 * is a hipStream_t passed as void* (NULL = the HIP default stream, as in every HIP API; this
 * is also what torch.cuda.current_stream().cuda_stream is for torch's default stream).
 */
#ifndef ORBX_H
#define ORBX_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    ORBX_OK = 0,
    ORBX_ERR_ARG = -1,         /* bad argument (NULL, non-positive size, level too small, ...) */
    ORBX_ERR_NO_DEVICE = -2,   /* no usable HIP device / kernel image for this GPU */
    ORBX_ERR_HIP = -3,         /* a HIP runtime call failed (see orbx_last_error) */
    ORBX_ERR_CAPACITY = -4,    /* caller-provided capacity too small */
    ORBX_ERR_UNSUPPORTED = -5  /* configuration outside the implemented range */
} orbx_status;

/* cv::KeyPoint layout the reference serialises (include/BoostArchiver.h:47-57): 28 bytes */
typedef struct {
    float x, y;       /* pt, in level-0 pixel units (pt *= mvScaleFactor[octave], :1095-1101) */
    float size;       /* (int)(31 * mvScaleFactor[octave]) */
    float angle;      /* IC_Angle, degrees [0,360) */
    float response;   /* FAST score */
    int32_t octave;
    int32_t class_id; /* -1 */
} orbx_keypoint_t;

typedef struct orbx_extractor orbx_extractor_t;

/* ---- extractor: replaces class ORBextractor (include/ORBextractor.h:45-111) ---------- */

/* ORBextractor::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
 * (src/ORBextractor.cc:410-470).  device = HIP device ordinal. */
int orbx_create(int nfeatures, float scale_factor, int nlevels, int ini_th_fast, int min_th_fast,
                int device, orbx_extractor_t **out);
int orbx_destroy(orbx_extractor_t *h);

/* Flavour of the OpenCV primitives behind the reference's calls.  The reference does not contain them (OpenCV, version unpinned:
 * CMakeLists.txt:52-58, README "2.4.11 and 3.2") and ships no vectors, so where OpenCV itself computes a primitive in two ways the
 * choice is a property of the reference BUILD this library stands in for.  It is fixed when the handle is created and never changes
 * afterwards (orbx_get_flavour reads it back); orbx_create = every field 0.
 *   gauss_rounding - cv::GaussianBlur(7x7, sigma 2) on 8U (src/ORBextractor.cc:1085-1086), rounding of the column pass, OpenCV <= 3.3:
 *     ORBX_GAUSS_ROUND_HALF_UP  (sum + 2^15) >> 16 on every column: the scalar FixedPtCastEx (builds without SSE2 / NEON column code)
 *     ORBX_GAUSS_ROUND_SSE2     x86 builds (SSE2 is baseline on x86-64): SymmColumnVec_32s8u rounds the columns x < (w & ~3) of a
 *                               level half to EVEN (_mm_cvtps_epi32); the last w % 4 columns take the scalar half-up code.
 *   The two differ at ~1 pixel in 131 072 (sum mod 65536 == 32768 with an even quotient).
 *     ORBX_GAUSS_FIXED_TAPS     OpenCV >= 3.4.1: the bit-exact 8-bit Gaussian (rows in ufixedpoint16, columns in ufixedpoint32, one
 *                               rounding (sum + 2^15) >> 16, scalar and SIMD code agree) - the arithmetic of HALF_UP on the seven Q8 taps
 *                               gauss_taps[] = { k0 (centre), k1, k2, k3 } the BUILD uses.  { 55, 49, 34, 18 } = cvRound(256 g_i), sum 257:
 *                               identical to HALF_UP (3.4.1 up to the error-diffused kernel); later releases spread the rounding error so
 *                               that the taps add up to 256 - { 56, 48, 34, 18 } by the left-to-right diffusion restated in
 *                               oracle.refvec.diffused_taps.  When in doubt the taps are FITTED from a reference-vector file's blurred
 *                               level (oracle.refvec.fit_gauss_taps; tests/golden/README.md).  k0 + 2 (k1 + k2 + k3) <= 257, k0 >= 1.
 *   Which one a given reference build follows is reported by the reference-vector consumer (tests/golden/README.md); all are
 *   hypotheses until vectors exist. */
#define ORBX_GAUSS_ROUND_HALF_UP 0
#define ORBX_GAUSS_ROUND_SSE2 1
#define ORBX_GAUSS_FIXED_TAPS 2
typedef struct {
    int32_t gauss_rounding;   /* ORBX_GAUSS_ROUND_* / ORBX_GAUSS_FIXED_TAPS */
    int32_t gauss_taps[4];    /* ORBX_GAUSS_FIXED_TAPS: Q8 taps, centre first; every other flavour: must be 0 */
    int32_t reserved[3];      /* must be 0 */
} orbx_flavour_t;
int orbx_create_flavoured(int nfeatures, float scale_factor, int nlevels, int ini_th_fast, int min_th_fast,
                          int device, const orbx_flavour_t *flavour, orbx_extractor_t **out);
int orbx_get_flavour(const orbx_extractor_t *h, orbx_flavour_t *out);

/* GetLevels / GetScaleFactor(s) / GetInverseScaleFactors / GetScaleSigmaSquares /
 * GetInverseScaleSigmaSquares (include/ORBextractor.h:62-83); arrays of nlevels floats,
 * any may be NULL.  features_per_level / umax expose mnFeaturesPerLevel and umax[16]. */
int orbx_get_levels(const orbx_extractor_t *h);
float orbx_get_scale_factor(const orbx_extractor_t *h);
int orbx_get_tables(const orbx_extractor_t *h, float *scale_factors, float *inv_scale_factors,
                    float *level_sigma2, float *inv_level_sigma2, int32_t *features_per_level,
                    int32_t *umax16);
/* upper bound of keypoints one image can produce (nfeatures + 3 per level) */
int orbx_max_keypoints(const orbx_extractor_t *h);

/* ORBextractor::operator()(image, mask, keypoints, descriptors) for one host image
 * (src/ORBextractor.cc:1043-1105).  img: 8-bit gray, `stride` bytes per row.  Writes up
 * to `cap` keypoints (28 B each) and descriptors (32 B each, row-major N x 32) into host
 * buffers and *n_out.  Empty image (w==0||h==0||img==NULL): returns ORBX_OK with
 * *n_out = 0 and outputs untouched (reference :1046-1047).  Synchronous. */
int orbx_extract(orbx_extractor_t *h, const uint8_t *img, int w, int hgt, int stride,
                 orbx_keypoint_t *kps, uint8_t *desc, int cap, int *n_out);

/* Batched many-frame mode on host buffers: B images of identical size.  imgs[b] points
 * at image b.  kps: B*cap entries, desc: B*cap*32 bytes, n_out: B counts.  Synchronous. */
int orbx_extract_batch(orbx_extractor_t *h, const uint8_t *const *imgs, int B, int w, int hgt,
                       int stride, orbx_keypoint_t *kps, uint8_t *desc, int cap, int *n_out);

/* Batched mode on DEVICE buffers (inputs already resident in HBM), asynchronous on
 * `stream`.  d_imgs: B images, image b at d_imgs + b*image_stride_bytes, rows `stride`
 * bytes apart.  d_kps [B][cap], d_desc [B][cap][32], d_counts [B] int32 are device
 * outputs; per-image layout is level-major exactly as the reference concatenates
 * (:1076-1104).  If a frame produces more than cap keypoints its count is clamped to cap
 * (cap >= orbx_max_keypoints() never clamps). */
int orbx_extract_batch_device(orbx_extractor_t *h, const uint8_t *d_imgs, int B, int w, int hgt,
                              int stride, size_t image_stride_bytes, orbx_keypoint_t *d_kps,
                              uint8_t *d_desc, int32_t *d_counts, int cap, void *stream);

/* Software pipelining across batches (optional).  Starts ComputePyramid (src/ORBextractor.cc:1107-1132) of the NEXT batch on a
 * side stream - `side_stream`, or a stream owned by the handle when that is NULL - into a second pyramid buffer, ordered behind
 * the FAST stage of the orbx_extract_batch_device call issued last on this handle: the memory-bound pyramid then runs beside that
 * call's latency-bound gather / quad-tree and its descriptor kernel instead of in front of the next call's FAST.  The next
 * orbx_extract_batch_device call with the SAME (d_imgs, B, w, hgt, stride, image_stride_bytes) takes that pyramid and skips its
 * own; any other call ignores it.
 * Contract: the images must be complete in HBM when this is called (it does not wait for the caller's main stream) and must stay
 * unchanged until that next call has been issued; extraction calls on one handle come from one stream.  Results are identical with
 * or without it. */
int orbx_extract_batch_device_prefetch(orbx_extractor_t *h, const uint8_t *d_imgs, int B, int w, int hgt, int stride,
                                       size_t image_stride_bytes, void *side_stream);

/* In-place input of the batched mode: the caller puts its frames where pyramid level 0 would be copied to, and the copy goes away
 * (one pass over every image per call: 60 MB read and 67 MB written per 128 images of 1241x376).
 * orbx_level0_layout: the layout, a pure function of the size and the levels (no HIP call, works without a GPU) - exactly what a handle
 * with these levels plans for level 0, and it refuses the sizes such a handle refuses (ORBX_ERR_ARG / ORBX_ERR_UNSUPPORTED, reason in
 * orbx_last_error).  An image is `prows` rows of `pstride` bytes; pixel (0,0) is at byte `pixel0_offset` = 19 * pstride + 19, pixel
 * (x, y) at pixel0_offset + y * pstride + x; images are at least `image_bytes` apart.  Everything of an image's bytes outside its w x h
 * pixels - the margins - is the caller's: its contents are unspecified, the library neither takes results from it nor writes it.
 * A producer that copies frames with a copy engine (hipMemcpy2DAsync, pitch = pstride) pays the same for this layout as for a dense one. */
typedef struct {
    int32_t pstride;         /* bytes from a row to the next (a multiple of 64) */
    int32_t prows;           /* rows of an image: hgt + 2 * 19 */
    uint64_t pixel0_offset;  /* byte offset of pixel (0,0) inside an image */
    uint64_t image_bytes;    /* bytes of one image, with the slack wide loads at its end may touch (a multiple of 256) */
} orbx_level0_layout_t;
int orbx_level0_layout(int w, int hgt, int nlevels, float scale_factor, orbx_level0_layout_t *out);
/* orbx_extract_batch_device on B images in that layout: image b starts at d_level0 + b * image_stride_bytes (64-byte aligned,
 * image_stride_bytes a multiple of 64 and >= image_bytes).  Level 0 is read where it is; the handle's pyramid block holds the levels >= 1.
 * Same outputs, bit for bit, as orbx_extract_batch_device on the same pixels.
 * Contract: the images must stay unchanged until everything that reads level 0 has FINISHED - this call, and the stereo matcher call that
 * works on its pyramid: orbm_stereo_batch_device, or the lagged orbm_stereo_batch_device_prev issued after the NEXT extraction call.
 * (orbx_extract_batch_device lets go of its images once the call itself has run.)  orbx_pyramid_host / orbx_pyramid_device of level 0
 * copy it into the pyramid block on demand and need the images unchanged as well.
 * The call copies level 0 after all - same results, no error - when the level-wide blur takes level 0 (ORBX_OPT_BLUR_FORM /
 * ORBX_OPT_BLUR_THRESHOLD), when the call - or the smallest chunk ORBX_OPT_CHUNKS cuts it into - has at most 4 images (the latency
 * forms of the pyramid start from the pyramid block) or when a developer option picks another pyramid form; the images are then free
 * when the call has run.
 * orbx_extract_batch_device_padded_prefetch: the companion of orbx_extract_batch_device_prefetch, with the same pairing rule (the next
 * padded call with the same arguments takes the pyramid built ahead). */
int orbx_extract_batch_device_padded(orbx_extractor_t *h, const uint8_t *d_level0, int B, int w, int hgt, size_t image_stride_bytes,
                                     orbx_keypoint_t *d_kps, uint8_t *d_desc, int32_t *d_counts, int cap, void *stream);
int orbx_extract_batch_device_padded_prefetch(orbx_extractor_t *h, const uint8_t *d_level0, int B, int w, int hgt,
                                              size_t image_stride_bytes, void *side_stream);

/* Two (default) or three pyramid buffers per handle.  With three, the pyramid built ahead gets a buffer of its own and the previous
 * call's pyramid stays valid across orbx_extract_batch_device_prefetch, so the pattern below may issue the prefetch of batch i+1
 * BEFORE orbm_stereo_batch_device_prev of batch i-1 on the side stream (the matcher then runs beside the descriptor kernel of batch i
 * instead of beside its quad-tree: better when there are many keypoints per image).  Costs one more pyramid buffer of HBM. */
int orbx_set_pyramid_buffers(orbx_extractor_t *h, int n);

/* Orders `stream` behind the FAST stage of the extraction call issued last on h (the point the pyramid built ahead waits for).
 * With orbm_stereo_batch_device_prev this lets a throughput pipeline run the stereo matcher of batch i-1 beside the gather /
 * quad-tree / descriptor kernels of batch i:
 *     orbx_extract_batch_device(h, batch i, main);  orbx_stream_wait_fast_stage(h, side);
 *     orbm_stereo_batch_device_prev(h, h, ... arrays of batch i-1 ..., side);
 *     orbx_extract_batch_device_prefetch(h, batch i+1, ..., side);      (same side stream: the matcher still reads the buffer) */
int orbx_stream_wait_fast_stage(orbx_extractor_t *h, void *stream);

/* The handle's own side stream (hipStream_t), for the pattern above.  HIP deals streams to a handful of hardware queues
 * round-robin, so a stream the caller creates may share its queue with the main stream and overlap nothing. */
void *orbx_side_stream(orbx_extractor_t *h);
/* The same, made sure not to share a hardware queue with main_stream (two streams on one queue run strictly in order and overlap
 * nothing): probed once with a 2-ms one-wave spin on main_stream and an empty kernel on the candidate, replaced by a fresh stream
 * if it queued behind the spin.  Call it once per handle with the stream the extraction calls will be issued on (every handle
 * after the first of a process is likely to need the replacement).  Returns the side stream to use. */
void *orbx_side_stream_for(orbx_extractor_t *h, void *main_stream);

/* mvImagePyramid[level] of image `b` of the last call (include/ORBextractor.h:85): copies
 * the inner level (padded=0) or the whole bordered buffer (padded=1, 19 px border,
 * BORDER_REFLECT_101) into dst (dst_stride bytes per row) and reports its size. dst may
 * be NULL to query the size only.  Synchronises the handle's last stream. */
int orbx_pyramid_host(orbx_extractor_t *h, int b, int level, int padded, uint8_t *dst, int dst_stride,
                      int *w, int *hgt);
/* Device view of the same level: pointer to the inner ROI's first pixel and its row stride. */
int orbx_pyramid_device(orbx_extractor_t *h, int b, int level, const uint8_t **d_ptr, int *w, int *hgt,
                        int *stride);

/* FAST candidates kept per level (what vToDistributeKeys holds, src/ORBextractor.cc:789-829) and keypoints DistributeOctTree returned
 * per level for image slot b of the last call: candidates[nlevels], keypoints[nlevels] (either may be NULL).  Read-only statistics. */
int orbx_level_counts(orbx_extractor_t *h, int b, int32_t *candidates, int32_t *keypoints);

/* Per-stage GPU time in ms, measured with HIP events recorded on the launch stream around
 * each stage of every batch call while profiling is enabled (a ring of event sets, so no
 * call ever waits for the GPU): [0] pyramid (k_pyr_*) [1] FAST cells (k_fast_cells)
 * [2] quad-tree (k_octree) [3] orientation+blur+descriptor (k_describe) [4] whole call.
 * orbx_get_stage_ms returns the AVERAGE per call since orbx_set_profiling(h,mode) and the number
 * of calls averaged (ncalls may be NULL).  mode 0: off; 1: all stage boundaries; 2: only the two events
 * around k_fast_cells ([1] is filled, the rest stays 0) - every recorded event idles the GPU for ~4.5 us,
 * so a throughput run brackets just the kernel whose duration it reports; 3: as 2, on every 4th call only (the average is over the
 * bracketed calls). */
#define ORBX_NUM_STAGES 5
/* Stage [1] is k_fast_strips (one wave per strip of four cells; levels whose cells are at most 32 px wide, batches that fill
 * the GPU) and / or k_fast_cells (one wave per cell; the other levels, small batches): which of them a batch of B images of
 * the planned size runs.  Same results either way.  A call is ONE chunk by default (ORBX_OPT_CHUNKS cuts a batch into up to
 * four chunks whose kernels overlap on the handle's side streams; the call keeps its stream semantics); the events of stage
 * [1] bracket the first chunk's launch, which covers *images_per_launch images (= B by default). */
int orbx_fast_kernels(const orbx_extractor_t *h, int B, int *strips, int *cells, int *images_per_launch);
int orbx_set_profiling(orbx_extractor_t *h, int enabled);
int orbx_get_stage_ms(orbx_extractor_t *h, float *ms5, int *ncalls);

/* ---- matchers: replace the hot ORBmatcher / Frame routines --------------------------- */

/* ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1649-1665): host, pure. */
int orbm_hamming(const uint8_t *a32, const uint8_t *b32);

/* All-pairs 256-bit Hamming distances on device: d_out[i*nb + j] (uint16) =
 * distance(d_a[i], d_b[j]).  Building block + bandwidth probe of the matchers. */
int orbm_hamming_matrix_device(const uint8_t *d_a, int na, const uint8_t *d_b, int nb,
                               uint16_t *d_out, void *stream);

/* Multi-GPU result exchange: pack the device outputs of B frames into ONE fixed-capacity record per
 * frame so that a step needs a single all-gather:
 *   [ cap x 28 B keypoints | cap x 32 B descriptors | cap x 4 B mvuRight | cap x 4 B mvDepth | int32 count | 12 B zero ]
 * record size = orbx_record_bytes(cap) = 68*cap + 16.  d_uright / d_depth may be NULL (monocular: zeros).  One kernel,
 * asynchronous on stream.  orb_slam2v2-1_amd/batching.py holds the matching unpack. */
int orbx_record_bytes(int cap);
int orbx_pack_records_device(const orbx_keypoint_t *d_kps, const uint8_t *d_desc, const float *d_uright,
                             const float *d_depth, const int32_t *d_counts, int B, int cap, uint8_t *d_records,
                             void *stream);

/* Frame::ComputeStereoMatches (src/Frame.cc:481-655) for B stereo frames.  Left/right
 * keypoints + descriptors + counts are the DEVICE outputs of two extractors (hl, hr) whose
 * pyramids of the same batch are still resident.  d_uright / d_depth: [B][cap] float
 * (mvuRight / mvDepth, -1 = no match).  mbf = baseline*fx, mb = mbf/fx (Frame.cc:114).
 * d_nmatch [B] (may be NULL) = number of surviving matches. Asynchronous on stream.
 * Frame b reads the pyramid of image slot left_slot0+b of hl and right_slot0+b of hr; hl and
 * hr may be the SAME handle when one extractor processed left and right images in one batch
 * (e.g. slots [0,B) left, [B,2B) right). */
int orbm_stereo_batch_device(orbx_extractor_t *hl, orbx_extractor_t *hr, int B,
                             int left_slot0, int right_slot0,
                             const orbx_keypoint_t *d_kl, const uint8_t *d_dl, const int32_t *d_nl,
                             const orbx_keypoint_t *d_kr, const uint8_t *d_dr, const int32_t *d_nr,
                             int cap, float mbf, float mb, float *d_uright, float *d_depth,
                             int32_t *d_nmatch, void *stream);

/* orbm_stereo_batch_device on the pyramids of the extraction call BEFORE the last one on hl / hr.  Valid only while that
 * pyramid still exists: the last extraction call took a pyramid built ahead (the two buffers swapped) and the next
 * orbx_extract_batch_device_prefetch has not been issued yet - otherwise ORBX_ERR_ARG.  Issue it on the stream that builds the
 * next pyramid afterwards (stream order protects the buffer). */
int orbm_stereo_batch_device_prev(orbx_extractor_t *hl, orbx_extractor_t *hr, int B,
                             int left_slot0, int right_slot0,
                             const orbx_keypoint_t *d_kl, const uint8_t *d_dl, const int32_t *d_nl,
                             const orbx_keypoint_t *d_kr, const uint8_t *d_dr, const int32_t *d_nr,
                             int cap, float mbf, float mb, float *d_uright, float *d_depth,
                             int32_t *d_nmatch, void *stream);
/* One stereo frame, host to host, in ONE call: the stereo Frame constructor's ExtractORB(left) || ExtractORB(right) followed by
 * ComputeStereoMatches (src/Frame.cc:78-84, 481-655).  Both images are extracted as one batch of two on h (a second extractor handle
 * is not needed), matched on the device and everything comes down behind one synchronisation.  kl / dl / uright / depth: left
 * keypoints, descriptors, mvuRight, mvDepth (cap entries each); kr / dr: right keypoints and descriptors; *nl, *nr, *nmatch counts.
 * More than cap keypoints: clamped, ORBX_ERR_CAPACITY.  Empty image: ORBX_OK with zero counts.  Synchronous. */
int orbx_stereo_frame(orbx_extractor_t *h, const uint8_t *left, const uint8_t *right, int w, int hgt, int stride,
                      float mbf, float mb, int cap, orbx_keypoint_t *kl, uint8_t *dl, int *nl, orbx_keypoint_t *kr,
                      uint8_t *dr, int *nr, float *uright, float *depth, int *nmatch);

/* The LATENCY form of the same call (round 5) - the shape the reference runs this path in: ONE stereo frame at a time, the next
 * frame needing this one's pose (src/Tracking.cc:275 -> Frame::Frame, src/Frame.cc:61-120).  Nothing is copied by a copy command:
 *  - left / right may be PINNED host memory (orbx_host_alloc, hipHostMalloc, hipHostRegister: the first kernel reads the pixels
 *    over the bus itself), device memory, or ordinary pageable memory (then the call stages them through a pinned buffer of the
 *    handle with one memcpy each - the price of a pageable cv::Mat; allocate capture buffers with orbx_host_alloc to avoid it);
 *  - the results are one fixed-layout record per frame that the LAST kernel writes to pinned host memory of the handle; *view
 *    points into it (host) and into the same record in HBM (d_*: what the device-resident matchers orbm_*_device take).
 * The handle keeps TWO records and alternates: the view of a call stays valid until the call after the next one on the same
 * handle (the previous frame's descriptors are what SearchByProjection(cur, last) reads, src/ORBmatcher.cc:1330-1472).
 * Results are those of orbx_stereo_frame bit for bit.  Empty image: ORBX_OK, zero counts, pointers NULL.  Synchronous. */
typedef struct {
    int32_t nl, nr, nmatch, cap;              /* keypoints left / right, stereo matches, rows allocated per array */
    const orbx_keypoint_t *kl, *kr;           /* host (pinned, owned by the handle) */
    const uint8_t *dl, *dr;                   /* 32 B per keypoint */
    const float *uright, *depth;              /* mvuRight, mvDepth of the left keypoints */
    const orbx_keypoint_t *d_kl, *d_kr;       /* the same arrays in HBM */
    const uint8_t *d_dl, *d_dr;
    const float *d_uright, *d_depth;
} orbx_stereo_view_t;
int orbx_stereo_frame_view(orbx_extractor_t *h, const uint8_t *left, const uint8_t *right, int w, int hgt, int stride,
                           float mbf, float mb, orbx_stereo_view_t *view);
/* ---- RGB-D frames: Tracking::GrabImageRGBD (src/Tracking.cc:315-345) + the RGB-D Frame constructor's feature part
 * (src/Frame.cc:119-171: ExtractORB, UndistortKeyPoints :419-449, ComputeStereoFromRGBD :658-679).
 * Camera: mK (fx fy cx cy), mDistCoef (k1 k2 p1 p2 [k3]; a 4-element mDistCoef has k3 = 0) and mbf.  Keypoints are undistorted
 * (cv::undistortPoints, restated in double) unless k1 == 0 - the reference's own test, even when p1 / p2 are not 0. */
typedef struct {
    float fx, fy, cx, cy;
    float k1, k2, p1, p2, k3;
    float mbf;
} orbx_rgbd_camera_t;
/* depth image element types: OpenCV's type codes CV_16U / CV_32F */
#define ORBX_DEPTH_U16 2
#define ORBX_DEPTH_F32 5

/* cvtColor(RGB2GRAY / BGR2GRAY / RGBA2GRAY / BGRA2GRAY) of B colour images in HBM, asynchronous on `stream`:
 * Y = (R*4899 + G*9617 + B*1868 + 8192) >> 14 (OpenCV's 8-bit RGB2Gray).  channels 3 or 4; rgb != 0: channel 0 is red, else blue.
 * Image b at d_color + b*image_stride_bytes, rows `stride` bytes apart; gray image b at d_gray + b*gray_image_stride_bytes, rows
 * gray_stride bytes apart. */
int orbx_gray_from_color_device(const uint8_t *d_color, int B, int w, int hgt, int channels, int rgb, int stride,
                                size_t image_stride_bytes, uint8_t *d_gray, int gray_stride, size_t gray_image_stride_bytes,
                                void *stream);
/* UndistortKeyPoints + ComputeStereoFromRGBD for the DEVICE outputs of orbx_extract_batch_device (d_kps [B][cap], d_counts [B]),
 * asynchronous on `stream`.  d_kun [B][cap] (mvKeysUn), d_uright / d_depth_out [B][cap] (mvuRight / mvDepth); rows past each frame's
 * count are not written.  Depth image b at d_depth + b*depth_image_stride_bytes, rows depth_stride bytes apart, w x hgt elements of
 * depth_type; the depth at a keypoint is d = imDepth(int(y), int(x)) at the DISTORTED position, converted as GrabImageRGBD does:
 * d = (float)raw * depth_map_factor unless depth_type is F32 and |depth_map_factor - 1| <= 1e-5.  d > 0: mvDepth = d,
 * mvuRight = kun.x - mbf/d; else (0, negative, NaN, outside the image) -1 / -1.  d_depth == NULL: the monocular constructor's tail
 * (src/Frame.cc:174-228): mvKeysUn and -1 / -1. */
int orbm_rgbd_batch_device(const orbx_keypoint_t *d_kps, const int32_t *d_counts, int B, int cap, const void *d_depth,
                           int depth_type, int w, int hgt, int depth_stride, size_t depth_image_stride_bytes,
                           float depth_map_factor, const orbx_rgbd_camera_t *cam, orbx_keypoint_t *d_kun, float *d_uright,
                           float *d_depth_out, void *stream);
/* One RGB-D frame host to host (synchronous): GrabImageRGBD's conversions + the RGB-D Frame constructor's feature part.
 * img: 8-bit, channels 1 (gray, used as is), 3 or 4 (rgb as above), `stride` bytes per row.  depth: w x hgt of depth_type,
 * depth_stride bytes per row, or NULL (monocular tail).  depth_map_factor: mDepthMapFactor (= 1 / DepthMapFactor of the settings).
 * Out (cap rows each): kp / desc (mvKeys, mDescriptors), kun (mvKeysUn), uright, depth_out (mvuRight, mvDepth), *n.
 * The colour conversion and the extraction run on the handle's stream with the gray image in handle-owned scratch, the depth image
 * goes up on a side stream meanwhile.  Empty image: ORBX_OK, *n = 0.  Bad channels, depth type or NULL camera: ORBX_ERR_ARG.
 * More than cap keypoints: clamped, ORBX_ERR_CAPACITY. */
int orbx_rgbd_frame(orbx_extractor_t *h, const uint8_t *img, int channels, int rgb, int w, int hgt, int stride,
                    const void *depth, int depth_type, int depth_stride, float depth_map_factor,
                    const orbx_rgbd_camera_t *cam, int cap, orbx_keypoint_t *kp, uint8_t *desc, int *n,
                    orbx_keypoint_t *kun, float *uright, float *depth_out);

/* ---- Stereo rectification of raw pairs: the stereo node's cv::initUndistortRectifyMap once per camera and cv::remap(INTER_LINEAR)
 * of both images per frame (ros_stereo.cc:106-107, 161-162), then Tracking::GrabImageStereo's cvtColor (src/Tracking.cc:275-310).
 * A rectifier holds one camera's maps on one device (DESIGN.md §3 items 9-11 restate the arithmetic).  It is immutable after
 * creation: any thread or stream may use it. */
typedef struct orbx_rectifier orbx_rectifier_t;
/* initUndistortRectifyMap(K, D, R, P3x3, Size(w, hgt), CV_32FC1): K, R, P3x3 row-major 3x3 (P3x3 = the first three columns of the
 * settings' P), D: nD = 4, 5 or 8 coefficients (k1 k2 p1 p2 [k3 [k4 k5 k6]]).  Map size 1..4095 each way.  A singular P3x3 * R,
 * another nD, a bad size or device: ORBX_ERR_ARG. */
int orbx_rectifier_create(const double K[9], const double *D, int nD, const double R[9], const double P3x3[9], int w, int hgt,
                          int device, orbx_rectifier_t **out);
int orbx_rectifier_destroy(orbx_rectifier_t *r);
/* The CV_32F maps (M1 = x, M2 = y) as initUndistortRectifyMap returns them, w * hgt floats each, row-major; either may be NULL. */
int orbx_rectifier_maps(const orbx_rectifier_t *r, float *mapx, float *mapy);
/* Output tiles, tiles that gather their taps from memory (the footprint does not fit in LDS), device bytes held.  Any may be NULL. */
int orbx_rectifier_info(const orbx_rectifier_t *r, int *tiles, int *gather_tiles, size_t *device_bytes);
/* remap(src, dst, M1, M2, INTER_LINEAR, BORDER_CONSTANT 0) of B raw 8-bit images in HBM, asynchronous on `stream`: images [0, B0)
 * through r0, [B0, B) through r1 (a rectifier no image uses may be NULL; both have one map size and device).  Source image b at
 * d_src + b*image_stride_bytes, sw x sh pixels of `channels` (1, 3, 4) bytes, rows `stride` bytes apart; the source may be larger or
 * smaller than the map.  Output: the map's size, gray (3 / 4 channels: RGB[A]/BGR[A]2GRAY of the remapped pixel, rgb != 0: channel 0
 * is red) at d_gray + b*gray_image_stride_bytes, rows gray_stride bytes apart. */
int orbx_rectify_device(const orbx_rectifier_t *r0, const orbx_rectifier_t *r1, int B0, const uint8_t *d_src, int B, int sw, int sh,
                        int channels, int rgb, int stride, size_t image_stride_bytes, uint8_t *d_gray, int gray_stride,
                        size_t gray_image_stride_bytes, void *stream);
/* orbx_stereo_frame on a RAW pair: both images (w x hgt, `channels` 1 / 3 / 4, rows `stride` bytes apart) go up once, are rectified
 * by rl / rr (map size w x hgt, the handle's device) into handle scratch in HBM and converted to gray, then extracted and matched as
 * orbx_stereo_frame does.  Results equal orbx_stereo_frame on the rectified gray pair.  NULL rectifier, bad channels, map size,
 * device or stride: ORBX_ERR_ARG.  Empty image: ORBX_OK with zero counts.  Synchronous. */
int orbx_stereo_frame_rectified(orbx_extractor_t *h, const orbx_rectifier_t *rl, const orbx_rectifier_t *rr, const uint8_t *left,
                                const uint8_t *right, int channels, int rgb, int w, int hgt, int stride, float mbf, float mb, int cap,
                                orbx_keypoint_t *kl, uint8_t *dl, int *nl, orbx_keypoint_t *kr, uint8_t *dr, int *nr, float *uright,
                                float *depth, int *nmatch);
/* The latency form on a raw pair: the images are read where they lie (pinned host or device memory; pageable memory is staged once
 * into pinned memory of the handle), rectified into handle scratch in HBM, then orbx_stereo_frame_view runs on the gray pair - the
 * same record, alternation and validity.  Errors as orbx_stereo_frame_rectified.  Synchronous. */
int orbx_stereo_frame_view_rectified(orbx_extractor_t *h, const orbx_rectifier_t *rl, const orbx_rectifier_t *rr, const uint8_t *left,
                                     const uint8_t *right, int channels, int rgb, int w, int hgt, int stride, float mbf, float mb,
                                     orbx_stereo_view_t *view);

/* ---- Dense RGB-D keyframe clouds: PointCloudMapping::generatePointCloud (src/pointcloudmapping.cc:83-114) and the
 * pcl::VoxelGrid<PointXYZRGBA> filter saveOctomap puts every keyframe's cloud through (:117-127); further
 * down the map's occupancy octree (the axis swap, octomap insertion and writeBinary, :198-278, items 14-15).  Plane segmentation,
 * whose result the reference never uses, and PCD input / output (:139-185) stay with the caller. */
typedef struct {
    float x, y, z;
    uint8_t b, g, r, a;   /* "b" is channel 0 of the colour image whatever its order, as the reference names it (:99-101) */
} orbx_cloud_point_t;     /* 16 bytes */
typedef struct orbx_cloudmapper orbx_cloudmapper_t;
/* PointCloudMapping(resolution): leaf = (float)resolution of voxel.setLeafSize; step: every step-th pixel of every step-th row (the
 * reference: 3); alpha: the a of every generated point (what PCL's default constructor leaves there differs between releases).
 * leaf <= 0, step < 1, alpha outside 0..255: ORBX_ERR_ARG, checked before the device is touched.  The mapper owns grow-only scratch
 * in HBM; its calls come from one stream at a time. */
int orbx_cloudmapper_create(float leaf, int step, int alpha, int device, orbx_cloudmapper_t **out);
int orbx_cloudmapper_destroy(orbx_cloudmapper_t *m);
/* points a w x hgt image can give at most: ceil(w / step) * ceil(hgt / step) (0: bad arguments) */
int orbx_cloud_capacity(int w, int hgt, int step);
/* generatePointCloud of B keyframes of one size and camera in HBM, asynchronous on `stream`.  Depth image b at d_depth +
 * b*depth_image_stride_bytes, rows depth_stride bytes apart, converted as GrabImageRGBD does (see orbm_rgbd_batch_device); colour image
 * b at d_color + b*color_image_stride_bytes, `channels` (3 or 4) bytes per pixel: b, g, r = bytes 0, 1, 2 of pixel n (the reference
 * indexes n*3 whatever the channel count, i.e. reads the wrong pixel of a 4-channel image).  A sample is kept unless d < 0.01 or
 * d > 10 (as doubles: a NaN depth is KEPT and gives a NaN point); z = d, x = (n - cx) * z / fx, y = (m - cy) * z / fy in float; then
 * p = Twc * (x, y, z, 1) in double, rounded to float.  Twc16: HOST, B x 16 doubles, row-major - the caller's
 * toSE3Quat(GetPose()).inverse().matrix(); it is read before the call returns.  Out: d_points [B][cap] in scan order, d_counts [B];
 * a count above cap is clamped. */
int orbx_cloud_generate_device(orbx_cloudmapper_t *m, const void *d_depth, int depth_type, int depth_stride,
                               size_t depth_image_stride_bytes, float depth_map_factor, const uint8_t *d_color, int channels,
                               int color_stride, size_t color_image_stride_bytes, int B, int w, int hgt, float fx, float fy, float cx,
                               float cy, const double *Twc16, orbx_cloud_point_t *d_points, int cap, int32_t *d_counts, void *stream);
/* VoxelGrid::applyFilter (leaf = the mapper's, downsample_all_data, no filter field) of B clouds in HBM, asynchronous on `stream`:
 * cloud b = the first min(d_counts[b], cap) rows of d_points + b*cap.  Points with a non-finite coordinate are dropped; one point per
 * occupied cell in ascending cell index, x y z and r g b a each the float sum over the cell's points in input order divided by their
 * number (colours truncated).  d_out [B][out_cap] (not d_points), d_out_counts [B]: clamped to out_cap; -1 where the grid has more
 * than INT32_MAX cells (PCL warns and returns its input: nothing is written). */
int orbx_cloud_voxel_device(orbx_cloudmapper_t *m, const orbx_cloud_point_t *d_points, const int32_t *d_counts, int B, int cap,
                            orbx_cloud_point_t *d_out, int out_cap, int32_t *d_out_counts, void *stream);
/* One keyframe host to host (synchronous): the images go up, then generate and filter as above.  raw_out (may be NULL) / n_raw (may
 * be NULL): the generated cloud; out / n: the filtered one - the generated one where the grid overflows, as PCL returns it; cap rows
 * each.  Empty image: ORBX_OK with zero counts.  More than cap points: clamped, ORBX_ERR_CAPACITY. */
int orbx_keyframe_cloud(orbx_cloudmapper_t *m, const uint8_t *color, int channels, int color_stride, const void *depth,
                        int depth_type, int depth_stride, float depth_map_factor, int w, int hgt, float fx, float fy, float cx, float cy,
                        const double *Twc16, int cap, orbx_cloud_point_t *raw_out, int *n_raw, orbx_cloud_point_t *out, int *n);

/* ---- The dense map's occupancy octree: what saveOctomap writes with tree.writeBinary (src/pointcloudmapping.cc:198-278), DESIGN.md
 * §3 items 14-15.  Every point goes through pcl::transformPointCloud with a float 4x4 (default: the reference's axis swap
 * x' = z, y' = -x, z' = -y), then octomap::OcTree(res).updateNode(point, true); writeBinary sets every occupied leaf to the clamping
 * maximum and prunes, so the file is a function of the SET of occupied depth-16 cells alone.  A point with a non-finite coordinate,
 * or whose key leaves [0, 65535] on an axis (|coordinate| beyond 32768 * res), is dropped and counted. */
typedef struct {
    uint16_t kx, ky, kz;   /* octomap key of the leaf's minimum corner: the low 16 - depth bits are zero */
    uint16_t depth;        /* 1 .. 16; 16: one cell of edge res */
} orbx_octree_leaf_t;      /* 8 bytes */
typedef struct {
    int64_t points_in;       /* points of all segments (counts clamped to [0, cap]) */
    int64_t points_dropped;  /* non-finite, or outside the tree */
    int64_t cells;           /* occupied depth-16 cells (distinct keys) */
    int64_t leaves;          /* leaves after pruning */
    int64_t tree_size;       /* OcTree::size() after pruning: inner nodes + leaves, root included; 0 for an empty map */
    int64_t data_bytes;      /* bytes after the header's "data" line: 2 per inner node */
    int32_t overflow;        /* 1: data_cap or leaf_cap was too small (the sizes above are still the true ones) */
    int32_t reserved;
} orbx_octree_info_t;        /* 56 bytes */
/* The tree of a map in HBM, asynchronous on `stream`; the host reads nothing between the kernels.  The map is the union of B
 * segments: the first clamp(d_counts[b], 0, cap) rows of d_points + b*cap - the layout orbx_cloud_voxel_device writes, so its output
 * feeds this call without a host trip.  (A voxel count of -1, "the grid overflowed, PCL returns its input", contributes nothing here:
 * a caller who wants that frame's unfiltered cloud in the map passes it as a segment of its own.)  B * cap <= 2^27.
 * M16f: HOST, 16 floats row-major, read before return; NULL: the axis swap.  Rows 0..2 are evaluated in float, every product and sum
 * rounded, left to right: x' = M00*x + M01*y + M02*z + M03.  res > 0 and finite, else ORBX_ERR_ARG (arguments are checked before the
 * device is touched).
 * d_data [data_cap] bytes: the .bt file's data section - two bytes per inner node in preorder.  d_leaves [leaf_cap] (NULL: skipped):
 * the leaves after pruning in preorder.  d_info: one orbx_octree_info_t.  Nothing is written at or past a capacity; a capacity that
 * is too small sets info.overflow, and the sizes reported are still the true ones.  Scratch: the mapper's, grow-only. */
int orbx_octree_device(orbx_cloudmapper_t *m, const orbx_cloud_point_t *d_points, const int32_t *d_counts, int B, int cap,
                       const float *M16f, double res, uint8_t *d_data, int64_t data_cap, orbx_octree_leaf_t *d_leaves, int64_t leaf_cap,
                       orbx_octree_info_t *d_info, void *stream);
/* Host to host, synchronous: the COMPLETE .bt file (header + data) of n points into out; *n_bytes: its size.  out_cap too small:
 * ORBX_ERR_CAPACITY with *n_bytes the size needed (out may be NULL when out_cap is 0).  n == 0: the header with "size 0" (no device
 * is needed for that).  info may be NULL. */
int orbx_octomap_bt(orbx_cloudmapper_t *m, const orbx_cloud_point_t *points, int n, const float *M16f, double res, uint8_t *out,
                    size_t out_cap, size_t *n_bytes, orbx_octree_info_t *info);
/* an upper bound of the file's size for n points: 2 * (15 n + 1) data bytes (every cell with a path of its own below the root) plus
 * 192 for the header; n < 0: 0 */
size_t orbx_octomap_bytes_bound(int64_t n);

/* Pinned host memory for image / capture buffers (cv::Mat can wrap it: cv::Mat(rows, cols, CV_8UC1, ptr)); NULL on failure. */
void *orbx_host_alloc(size_t bytes);
void orbx_host_free(void *p);

/* Host-buffer convenience for one frame (synchronous); pyramids come from hl / hr, which
 * must have just extracted the left / right image (image slot 0). */
int orbm_stereo(orbx_extractor_t *hl, orbx_extractor_t *hr,
                const orbx_keypoint_t *kl, const uint8_t *dl, int nl,
                const orbx_keypoint_t *kr, const uint8_t *dr, int nr,
                float mbf, float mb, float *uright, float *depth, int *nmatch);

/* Frame lookup grid geometry (src/Frame.cc:90-105, 397-407; include/Frame.h:37-38) */
typedef struct {
    float min_x, min_y, max_x, max_y; /* mnMinX, mnMinY, mnMaxX, mnMaxY */
    float inv_w, inv_h;               /* mfGridElementWidthInv, mfGridElementHeightInv */
} orbm_grid_geom_t;

/* ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)
 * (src/ORBmatcher.cc:405-520) on host arrays (undistorted keypoints).  prev_matched
 * [2*n1] (x,y) is updated in place; matches12[n1] out; *nmatches out. */
int orbm_search_for_initialization(const orbx_keypoint_t *k1, const uint8_t *d1, int n1,
                                   const orbx_keypoint_t *k2, const uint8_t *d2, int n2,
                                   const orbm_grid_geom_t *g2, float *prev_matched, int32_t *matches12,
                                   int window, float nnratio, int check_orientation, int device,
                                   int *nmatches);

/* ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th)
 * (src/ORBmatcher.cc:45-129), map points gathered into flat arrays by the C++ wrapper. */
typedef struct {
    int32_t in_view;          /* mbTrackInView && !isBad() */
    float proj_x, proj_y, proj_xr; /* mTrackProjX/Y/XR */
    int32_t level;            /* mnTrackScaleLevel */
    float view_cos;           /* mTrackViewCos */
    int32_t observations;     /* Observations() */
} orbm_mappoint_t;
/* frame_mp[n] in/out: index of the list's map point held by keypoint i, -1 none,
 * -2 = held by a map point outside the list whose Observations() is ext_obs[i]. */
int orbm_search_by_projection_mp(const orbx_keypoint_t *kun, const uint8_t *desc, const float *uright, int n,
                                 const orbm_grid_geom_t *g, const float *scale_factors, int nlevels,
                                 const orbm_mappoint_t *mps, const uint8_t *mp_desc, int m,
                                 int32_t *frame_mp, const int32_t *ext_obs, float th, float nnratio,
                                 int device, int *nmatches);

/* ORBmatcher::SearchByProjection(Frame &cur, const Frame &last, th, bMono)
 * (src/ORBmatcher.cc:1330-1472). */
typedef struct {
    int32_t has_mp;        /* mvpMapPoints[i] && !mvbOutlier[i] */
    float wx, wy, wz;      /* GetWorldPos() */
    int32_t observations;  /* Observations() */
    int32_t octave;        /* LastFrame.mvKeys[i].octave */
    float angle;           /* LastFrame.mvKeysUn[i].angle */
} orbm_lastpoint_t;
typedef struct { float fx, fy, cx, cy, mbf, mb; } orbm_camera_t;
/* cur_mp[n] in/out: index i of the last-frame keypoint whose map point keypoint j holds. */
int orbm_search_by_projection_frame(const orbx_keypoint_t *kun, const uint8_t *desc, const float *uright,
                                    int n, const orbm_grid_geom_t *g, const float *scale_factors,
                                    int nlevels, const orbm_camera_t *cam, const float *Tcw_cur16,
                                    const float *Tcw_last16, const orbm_lastpoint_t *last,
                                    const uint8_t *last_desc, int nlast, int32_t *cur_mp,
                                    const int32_t *ext_obs, float th, int mono, int check_orientation,
                                    int device, int *nmatches);

/* Device-resident form for a tracking front-end (Tracking::TrackWithMotionModel, src/Tracking.cc:1010-1041): the current
 * frame's keypoints, descriptors and mvuRight are the DEVICE outputs of orbx_extract_batch_device / orbm_stereo_batch_device
 * (first n entries of the frame's rows) and d_last_desc the previous frame's descriptor rows, still in HBM; only the
 * per-keypoint map-point records (`last`, 28 B each), the poses and the holders cross the bus.  The kernels run on
 * `stream`, i.e. behind the kernels that produce the arrays; the call returns when the results are on the host.
 * Same results as orbm_search_by_projection_frame. */
int orbm_search_by_projection_frame_device(const orbx_keypoint_t *d_kun, const uint8_t *d_desc, const float *d_uright,
                                           int n, const orbm_grid_geom_t *g, const float *scale_factors,
                                           int nlevels, const orbm_camera_t *cam, const float *Tcw_cur16,
                                           const float *Tcw_last16, const orbm_lastpoint_t *last,
                                           const uint8_t *d_last_desc, int nlast, int32_t *cur_mp,
                                           const int32_t *ext_obs, float th, int mono, int check_orientation,
                                           int device, int *nmatches, void *stream);

/* ---- the step before SearchByProjection(F, MPs) — Frame::isInFrustum
 * (src/Frame.cc:284-340) for all local map points at once (Tracking::SearchLocalPoints,
 * src/Tracking.cc:1290-1340).  A point's tracking variables come back as orbm_mappoint_t. */
typedef struct {
    int32_t valid;                      /* candidate: not already matched in this frame, !isBad() (:1306-1317) */
    float wx, wy, wz;                   /* GetWorldPos() */
    float nx, ny, nz;                   /* GetNormal() */
    float max_distance, min_distance;   /* mfMaxDistance, mfMinDistance (invariance range = 1.2x / 0.8x) */
    int32_t observations;               /* Observations(), copied to the output record */
} orbm_worldpoint_t;
/* MapPoint::PredictScale (src/MapPoint.cc:414-429) is ceil(log(ratio)/mfLogScaleFactor) with the C
 * library's float log, which a GPU cannot reproduce bit for bit at level boundaries.  The device
 * therefore compares ratio = mfMaxDistance/dist with nlevels-1 float thresholds that this HOST function
 * finds by bisection with the host's own logf: thresholds[k] = the smallest float r with
 * ceil(logf(r)/log_scale_factor) >= k+1.  Level = number of thresholds <= ratio (exact wherever logf is
 * monotonic).  No GPU needed. */
int orbm_predict_scale_thresholds(float log_scale_factor, int nlevels, float *thresholds);
/* Tcw16: row-major 4x4 camera pose; g: image bounds mnMinX..mnMaxY; out[m] as Frame::isInFrustum leaves
 * mbTrackInView / mTrackProjX / mTrackProjXR / mTrackProjY / mnTrackScaleLevel / mTrackViewCos. */
int orbm_is_in_frustum(const orbm_worldpoint_t *pts, int m, const float *Tcw16, const orbm_camera_t *cam,
                       const orbm_grid_geom_t *g, float viewing_cos_limit, const float *thresholds, int nlevels,
                       orbm_mappoint_t *out, int device);
/* isInFrustum + SearchByProjection(F, MPs) without the host round trip of the projections
 * (Tracking::SearchLocalPoints).  proj_out[m] (may be NULL) receives the isInFrustum records. */
int orbm_search_local_points(const orbx_keypoint_t *kun, const uint8_t *desc, const float *uright, int n,
                             const orbm_grid_geom_t *g, const float *scale_factors, int nlevels,
                             const orbm_worldpoint_t *pts, const uint8_t *mp_desc, int m, const float *Tcw16,
                             const orbm_camera_t *cam, float viewing_cos_limit, const float *thresholds,
                             int32_t *frame_mp, const int32_t *ext_obs, float th, float nnratio, int device,
                             int *nmatches, orbm_mappoint_t *proj_out);

/* orbm_search_local_points with the frame's keypoints / descriptors / mvuRight already in HBM (see
 * orbm_search_by_projection_frame_device); the map points' records and descriptors come from the host map. */
int orbm_search_local_points_device(const orbx_keypoint_t *d_kun, const uint8_t *d_desc, const float *d_uright, int n,
                                    const orbm_grid_geom_t *g, const float *scale_factors, int nlevels,
                                    const orbm_worldpoint_t *pts, const uint8_t *mp_desc, int m, const float *Tcw16,
                                    const orbm_camera_t *cam, float viewing_cos_limit, const float *thresholds,
                                    int32_t *frame_mp, const int32_t *ext_obs, float th, float nnratio, int device,
                                    int *nmatches, orbm_mappoint_t *proj_out, void *stream);

/* Generic projected-window matcher: the common core of the reference's SearchByProjection
 * family once the caller has projected its map points.  For every valid
 * query, in order: candidates = Frame::GetFeaturesInArea(u, v, radius, min_level, max_level)
 * (src/Frame.cc:342-395); a candidate is skipped when its slot already has a blocking holder
 * (and, if ur_tol >= 0, when uright[j] > 0 && |ur_c - uright[j]| > ur_tol); the first minimum
 * of the Hamming distance wins; if it is <= max_dist, holder[best] = query index, nmatches++,
 * and with check_orientation the match enters the 30-bin rotation histogram
 * (query angle - keypoint angle) whose bins outside the three maxima are undone at the end
 * (holder = -1, nmatches--), exactly as src/ORBmatcher.cc:1549-1597 does.
 * holder[n] in/out: -1 empty, >= 0 index of the query holding the slot, -2 held from outside
 * (ext_blocks[j] != 0 says whether that holder blocks; NULL = it blocks).  A query's own
 * claim blocks later queries iff queries[q].blocks != 0.
 * ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist)
 * (src/ORBmatcher.cc:1474-1601) = projection + MapPoint::PredictScale on the host
 * (orb_slam2v2-1_amd/host/ORBmatcher.cc) + this call with blocks = 1, max_dist = ORBdist. */
typedef struct {
    int32_t valid;
    float u, v, radius;
    int32_t min_level, max_level;
    float angle;      /* orientation of the query's own keypoint (pKF->mvKeysUn[i].angle) */
    int32_t blocks;
    float ur_c, ur_tol;
} orbm_window_query_t;
/* g_assign (both calls below): a KeyFrame keeps the cell lists its Frame built with float bounds
 * (src/KeyFrame.cc:41,53) but queries them with int-truncated bounds (include/KeyFrame.h:199-202,
 * src/KeyFrame.cc:577-589): pass the Frame's geometry here and the KeyFrame's in g.  NULL = g. */
int orbm_match_windows(const orbx_keypoint_t *kun, const uint8_t *desc, const float *uright, int n,
                       const orbm_grid_geom_t *g, const orbm_grid_geom_t *g_assign,
                       const orbm_window_query_t *queries, const uint8_t *query_desc,
                       int m, int32_t *holder, const int32_t *ext_blocks, int max_dist, int check_orientation,
                       int device, int *nmatches);

/* Stateless projected-window search: the matching core of ORBmatcher::Fuse (both overloads,
 * src/ORBmatcher.cc:827-977, 979-1102) and ORBmatcher::SearchBySim3 (:1104-1328), whose queries
 * never read what an earlier query wrote.  For every valid query: candidates =
 * KeyFrame::GetFeaturesInArea(u, v, radius) (src/KeyFrame.cc:572-611, same cells and order as
 * Frame's) with octave in [min_level, max_level] (the callers pass [pred-1, pred]); with
 * inv_level_sigma2 != NULL each candidate must also pass Fuse's reprojection gate (:916-940):
 * uright[j] >= 0 ? (ex^2+ey^2+er^2)*inv_level_sigma2[octave] <= 7.8, er = ur_c - uright[j]
 *               : (ex^2+ey^2)*inv_level_sigma2[octave] <= 5.99      (uright NULL = all mono).
 * Out: best_idx[m] = first minimum of the Hamming distance in scan order (-1: no candidate),
 * best_dist[m] (256 when none).  The caller applies its own threshold (TH_LOW / TH_HIGH) and
 * map-point bookkeeping (orb_slam2v2-1_amd/host/ORBmatcher.cc). angle, blocks, ur_tol unused.
 * An INVALID query (a point that is bad, already found or already in the keyframe, or that projects outside) answers best_idx -1,
 * best_dist 256, so Fuse(pKF, Scw, ..)'s vpReplacePoint stays null for it; SearchBySim3 passes the MAP POINT's descriptor of each
 * slot as query_desc, not the keyframe's own row, and accepts a pair only when both directions name each other. */
int orbm_best_in_windows(const orbx_keypoint_t *kun, const uint8_t *desc, const float *uright, int n,
                         const orbm_grid_geom_t *g, const orbm_grid_geom_t *g_assign,
                         const orbm_window_query_t *queries, const uint8_t *query_desc,
                         int m, const float *inv_level_sigma2, int nlevels, int32_t *best_idx, int32_t *best_dist,
                         int device);

/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:252-317), batched over map points
 * (SURVEY §8(f) rank 4).  Map point p owns the descriptors desc[offsets[p] .. offsets[p+1]) (the rows
 * of its non-bad observing keyframes, in std::map iteration order).  For each row i: all Hamming
 * distances to the point's rows (itself included, 0), median = sorted[(size_t)(0.5*(N-1))]; the FIRST
 * row with the least median wins.  Out: best_row[p] (index inside the point's block, -1 if it has no
 * rows), best_median[p] (may be NULL).  The caller copies row best_row[p] into mDescriptor. */
int orbm_distinctive_descriptors(const uint8_t *desc, const int32_t *offsets, int npoints, int32_t *best_row,
                                 int32_t *best_median, int device);

/* Per-handle options: which of several kernels / launch arrangements with IDENTICAL results a handle uses.  State of the handle
 * (no process-global switch exists: two handles on two threads may run with different options); set between calls, from the thread
 * that issues the handle's calls.  Defaults (every value 0) are the measured-fastest choices; the tests use the others to cover
 * every kernel against the oracle.  Unknown keys / values: ORBX_ERR_ARG.
 *   ORBX_OPT_PYR_TILE      3   tile size of the fused pyramid kernel at the coarsest level (0 = 64; takes effect at the next plan)
 *   ORBX_OPT_OCTREE_FORM   4   1 = quad-tree by the exact form alone, 2 = every level by the multi-workgroup form, 3 = no level by it
 *                              (default: levels with >= 600 FAST cells when the batch is at most 4 images)
 *   ORBX_OPT_PYRAMID_FORM  5   1 = pyramid by the one-launch fused kernel, 3 = levels 3.. by it (default: one launch per level)
 *   ORBX_OPT_FAST_FORM     6   1 = every level's FAST by k_fast_cells, 2 = ... with run-time tile strides, 3 = k_fast_strips even for
 *                              a small batch (default: by batch size)
 *   ORBX_OPT_CHUNKS        8   n >= 2: a batch is cut into n chunks (<= 4) on the handle's side streams (default one)
 *   ORBX_OPT_IGNORE_AHEAD  9   1 = pyramids built ahead are ignored
 *   ORBX_OPT_PREFETCH_GATE 10  where a pyramid built ahead may start: 0 behind FAST, 1 behind the quad-tree, 2 behind the descriptors,
 *                              3 together with FAST (pays when the quad-tree launch fills the GPU more than once and nothing else runs
 *                              beside FAST: pipeline.FrontEnd picks it for such mono batches)
 *   ORBX_OPT_OCTREE_WIDTH  11  quad-tree kernels in the 1024-thread build never (1) / always (2) (default: by image size)
 *   ORBX_OPT_NO_ORDER_KERNEL 12  1 = no ordering kernel in front of the FAST stage's start event
 *   ORBX_OPT_BLUR_FORM     13  1 = no level blurred as a whole, 2 = every level (orbx_debug_blurred_level); 14 = the rule's threshold
 *   ORBX_OPT_SPLIT_CALL    15  a >= 2: quad-tree of levels [0, a) on a second stream beside quad-tree + descriptors of the others
 *   ORBX_OPT_ROW_PRETEST   16  corner-sparse FAST path of k_fast_strips never (1) / on every level (2) (default: by the previous
 *                              call's candidate density)
 *   ORBX_OPT_GATHER        18  1 = k_gather + compacted key arrays instead of the quad-tree reading the FAST cell lists in place
 *   ORBX_OPT_EARLY_OCTREE  19  a >= 2: strips of levels [0, a) launched first, their quad-tree beside the FAST of the others
 *   ORBX_OPT_SPARSE_FORM   20  corner-sparse levels: 0 = rows of 128 pixels that cannot hold a corner are skipped inside k_fast_strips
 *                              (default), 1 = k_fast_strips_sparse (the pixel pairs that pass the five-pixel bound are queued and
 *                              scored 64 at a time), 2 = the same compaction inside the cell kernel; 1 and 2 measured no faster
 *   ORBX_OPT_DESC_LDS_PAD  21  KB of unused LDS per k_describe workgroup: fewer of them resident per CU, more wave slots for the
 *                              kernels of a neighbouring stream (tuning of the pipelined step; default 0)
 *   ORBX_OPT_PYR_ROWS      22  output rows per wave of k_pyr_level: 1 = always 8, 2 = always 16 (default: 16 while the level gives
 *                              every SIMD several waves, else 8).  2 only pays up to scale factor 1.25: beyond it 16 output rows
 *                              need more than the 22 source rows the form fetches and every band takes the row-by-row path
 *                              (correct, much slower than the 8-row form)
 *   ORBX_OPT_OCT_HIST      23  quad-tree input of batches of up to four images: 0 = the FAST stage histograms its emissions at the L2
 *                              and k_octree_pyr loads the histogram (no key sweep on one CU: the latency form, default), 1 = never
 *   ORBX_OPT_PAD_FORM      24  level 0 (copy of the input + copyMakeBorder): 0 = source rows staged in LDS for batches of up to four
 *                              images (each input byte read once, aligned: the input of a latency call sits in pinned host memory),
 *                              1 = never (k_pyr_pad: unaligned 16-byte chunks), 2 = always
 *   ORBX_OPT_PYR_CHAINS    25  levels >= 1 of batches of up to four images: 0 = in chains of up to four levels per launch (k_pyr_chain:
 *                              a tile's intermediate levels stay in LDS - per-level launches of one or two images are latency-bound),
 *                              1 = one launch per level as in a large batch, 2 / 3 = chains of up to four / seven levels.  ORBX_OPT_PYRAMID_FORM = 4
 *                              forces the chains at any batch size
 *   ORBX_OPT_OCT_SLICES    26  quad-tree of a batch: 1 = the key sweep of a level with >= 600 FAST cells is shared by two workgroups, >= 1600
 *                              by four (partial histograms summed by the last to arrive); 0 = one workgroup per level (default: the
 *                              shared form is faster alone and slower inside the pipelined step)
 *   ORBX_OPT_STREAM_SYNC   27  orbx_stereo_frame_view: 0 = the host polls the completion word the last kernel stores behind the record (the
 *                              stream wait as the fall-back), 1 = it waits for the stream
 * Keys 0, 1 and 7 (stop a kernel after phase n: outputs incomplete) exist only in a library built with -DORBX_DEVELOPER
 * (tools/octree_phase_probe.py); the default build refuses them. */
#define ORBX_OPT_PYR_TILE 3
#define ORBX_OPT_OCTREE_FORM 4
#define ORBX_OPT_PYRAMID_FORM 5
#define ORBX_OPT_FAST_FORM 6
#define ORBX_OPT_CHUNKS 8
#define ORBX_OPT_IGNORE_AHEAD 9
#define ORBX_OPT_PREFETCH_GATE 10
#define ORBX_OPT_OCTREE_WIDTH 11
#define ORBX_OPT_NO_ORDER_KERNEL 12
#define ORBX_OPT_BLUR_FORM 13
#define ORBX_OPT_BLUR_THRESHOLD 14
#define ORBX_OPT_SPLIT_CALL 15
#define ORBX_OPT_ROW_PRETEST 16
#define ORBX_OPT_GATHER 18
#define ORBX_OPT_EARLY_OCTREE 19
#define ORBX_OPT_SPARSE_FORM 20
#define ORBX_OPT_DESC_LDS_PAD 21
#define ORBX_OPT_PYR_ROWS 22
#define ORBX_OPT_OCT_HIST 23
#define ORBX_OPT_PAD_FORM 24
#define ORBX_OPT_PYR_CHAINS 25
#define ORBX_OPT_OCT_SLICES 26
#define ORBX_OPT_STREAM_SYNC 27
#define ORBX_NUM_OPTIONS 32
int orbx_set_option(orbx_extractor_t *h, int key, int value);
int orbx_get_option(const orbx_extractor_t *h, int key, int *value);
/* The guided-search matchers keep their scratch per host thread, and so their options: ORBM_OPT_EXACT_KERNELS = 1 makes the
 * calling thread's matcher calls take the exact one-workgroup kernels instead of candidate search + resolution; ORBM_OPT_RESOLVER
 * = 1 makes the resolution the single-wave speculative walk of rounds 1-4 instead of the whole-workgroup fixed-point iteration
 * (k_resolve_par, the default since round 5).  Identical results whatever the setting; the tests run all three.  Thread-local. */
#define ORBM_OPT_EXACT_KERNELS 2
#define ORBM_OPT_RESOLVER 3
#define ORBM_OPT_STREAM_SYNC 4   /* 1 = a guided search waits for its stream (hipStreamSynchronize); 0 (default) = it polls the completion word its
                                   * last kernel stores behind the results in pinned memory, with the stream wait as the fall-back after a few ms */
int orbm_set_thread_option(int key, int value);
/* The read-only stage hooks the staged parity tests look through (orbx_debug_* / orbm_debug_*) are NOT part of this library: they
 * exist in the developer build only (liborbx_hip_dev.so, -DORBX_DEVELOPER) and are declared in include/orbx_dev.h. */

/* ---- misc ---------------------------------------------------------------------------- */
/* ---- DBoW2 vocabulary descent and the BoW-guided matchers.
 * Vocabulary = the tree of Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:310-340 (nodes: parent, children in id
 * order, 32-byte FORB descriptor, weight; leaves are words, numbered in node-id order) held on the GPU. */
typedef struct orbv_vocabulary orbv_vocabulary_t;
/* nnodes includes the root (node 0, no descriptor).  parent[i] < i for i >= 1.  is_leaf[i]: the loader's nIsLeaf
 * flag (word ids follow it); a node is treated as a leaf by the descent iff it has no children (Node::isLeaf). */
int orbv_create(int k, int L, int scoring, int weighting, int nnodes, const int32_t *parent, const uint8_t *is_leaf,
                const uint8_t *desc, const double *weight, int device, orbv_vocabulary_t **out);
/* TemplatedVocabulary::loadFromTextFile (:1351-1436, the ORBvoc.txt format).  Difference: the reference's
 * `while(!f.eof())` loop turns the file's trailing empty line into one more child of the root with an
 * UNINITIALISED descriptor (undefined behaviour); empty lines are skipped here. */
int orbv_load_text(const char *path, int device, orbv_vocabulary_t **out);
void orbv_destroy(orbv_vocabulary_t *v);
int orbv_info(const orbv_vocabulary_t *v, int *k, int *L, int *scoring, int *weighting, int *nnodes, int *nwords);
/* transform(feature, word_id, weight, nid, levelsup) of TemplatedVocabulary.h:1230-1271 for n descriptors:
 * at every level the child with the smallest FORB::distance (first minimum in child order) until a leaf.
 * word_id[n], node_id[n] (the node on the path at level L - levelsup; 0 when that level is <= 0), weight[n].
 * The BowVector / FeatureVector maps are filled from these on the host, in feature order
 * (orb_slam2v2-1_amd/host/ORBVocabulary.h), because their double sums depend on that order. */
int orbv_transform(const orbv_vocabulary_t *v, const uint8_t *desc, int n, int levelsup, int32_t *word_id,
                   int32_t *node_id, double *weight);

/* ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...) (src/ORBmatcher.cc:159-288) and SearchByBoW(KeyFrame*, KeyFrame*,
 * ...) (:522-655) after the caller has intersected the two FeatureVectors: node j pairs the query features
 * q_items[node_qstart[j] .. node_qstart[j+1]) with the candidate features c_items[node_cstart[j] .. ).  Queries are
 * visited in that order; candidates in list order; a query needs q_valid (map point present and not bad), a
 * candidate needs c_valid (NULL = all valid) and must not have been taken by an earlier query; accept iff
 * best <= max_dist && (float)best < nnratio * (float)second (second = smallest distance among the other
 * candidates, 256 if none); with check_orientation the matches outside the three largest 30-degree bins of
 * (q_angle - c_angle) are dropped at the end.  A feature belongs to one node only, so nodes are independent:
 * one wavefront per node; a feature index that appears twice in q_items or twice in c_items is ORBX_ERR_ARG.
 * A node may hold at most 4096 candidates (one taken-bit each in a 64-bit register per lane): more is
 * ORBX_ERR_UNSUPPORTED.  On either error match_q is all -1 and *nmatches is 0.
 * match_q[nq]: candidate feature index or -1. */
int orbm_search_by_bow(const uint8_t *q_desc, const float *q_angle, const uint8_t *q_valid, int nq,
                       const uint8_t *c_desc, const float *c_angle, const uint8_t *c_valid, int nc,
                       const int32_t *node_qstart, const int32_t *q_items, const int32_t *node_cstart,
                       const int32_t *c_items, int nnodes, int max_dist, float nnratio, int check_orientation,
                       int32_t *match_q, int *nmatches, int device);

/* ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:657-825) on the intersected node lists (same layout as
 * orbm_search_by_bow).  flags: bit 0 = usable (query: no map point yet :703-704 and, with bOnlyStereo, stereo
 * :708-710; candidate: no map point :724-725 and the stereo rule :729-731), bit 1 = mvuRight >= 0.  For each
 * usable query, over the usable candidates of its node not taken by an earlier query, in list order:
 * dist <= TH_LOW and dist <= best so far (:737), then - both monocular - the candidate must be at least
 * sqrt(100*scale_factors[octave2]) away from the epipole (ex, ey) (:742-748), then CheckDistEpipolarLine
 * (:140-157: squared distance to the line x1'F12 < 3.84*level_sigma2[octave2]); a passing candidate becomes the
 * best — so among equal distances the LAST passing one wins.  F12_9: row-major 3x3.  Rotation consistency as in
 * orbm_search_by_bow, and so are the limits: a repeated index in q_items or in c_items is ORBX_ERR_ARG, more than
 * 4096 candidates in one node ORBX_ERR_UNSUPPORTED, match_q all -1 and *nmatches 0 on either.
 * match_q[nq]: candidate feature index or -1. */
int orbm_search_for_triangulation(const orbx_keypoint_t *kp1, const uint8_t *q_desc, const uint8_t *q_flags, int nq,
                                  const orbx_keypoint_t *kp2, const uint8_t *c_desc, const uint8_t *c_flags, int nc,
                                  const int32_t *node_qstart, const int32_t *q_items, const int32_t *node_cstart,
                                  const int32_t *c_items, int nnodes, const float *F12_9, float ex, float ey,
                                  const float *scale_factors, const float *level_sigma2, int nlevels, int max_dist,
                                  int check_orientation, int32_t *match_q, int *nmatches, int device);

/* ---- the keyframe database: ORB_SLAM2::KeyFrameDatabase (src/KeyFrameDatabase.cc:31-309) over BoW vectors, and
 * TemplatedVocabulary::score with L1Scoring (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68), the only scoring built.
 * A BoW vector is the content of a DBoW2::BowVector: n pairs (word id, value), ids strictly ascending.
 * A keyframe is named by the caller's id, 0 .. ORBV_DB_MAX_KF_ID (the id -> slot table is an array; a larger id is
 * ORBX_ERR_UNSUPPORTED, a negative one ORBX_ERR_ARG).  A query holds at most ORBV_DB_MAX_QUERY words (its ids are staged in
 * the LDS of every workgroup; more is ORBX_ERR_UNSUPPORTED).  No inverted file is kept: a query is intersected with every
 * keyframe of the database, one wavefront each, and the reference's list order - ascending (smallest common word,
 * position in that word's list) - is rebuilt from a sequence number every add stamps (erase keeps the relative order of
 * a list, so position = order of the add calls; a re-add after erase gets a new number).  Arguments are checked on the
 * host before any HIP call.  A handle owns its memory (entry pool, growing by doubling; slot table; one pinned result
 * buffer) and one stream; calls on one handle are serialised by a mutex inside it (the reference locks mMutex), different
 * handles run concurrently.  The pool space and the slot of an erased keyframe are not reclaimed before orbv_db_clear.
 * The reference's query stamps (mnLoopQuery == pKF->mnId, mnRelocQuery == F->mnId) are not modelled, so no call takes a
 * query id: they misbehave only for a repeated query id and for id 0 against fresh keyframes, which DetectLoop (no query
 * for the first ten keyframes) and Relocalization (frame 0 cannot relocalise) never produce. */
#define ORBV_DB_MAX_KF_ID ((1 << 20) - 1)
#define ORBV_DB_MAX_QUERY 8192
#define ORBV_DB_MAX_COVISIBLE 10
typedef struct orbv_db orbv_db_t;
/* one LISTED keyframe of a query (lKFsSharingWords), in list order.  flags: bit 0 = scored (words > minCommonWords), bit 1 =
 * entered lScoreAndMatch.  score: (float)score when scored; else 0 for a loop query and the keyframe's mRelocScore for a
 * relocalisation query.  acc_score / best_kf: the covisibility accumulation, 0 / -1 without bit 1. */
typedef struct {
    int32_t kf_id, words;
    uint32_t flags;
    float score, acc_score;
    int32_t best_kf;
} orbv_db_hit_t;
/* ORBVocabulary::score(v1, v2) = L1Scoring::score (ScoringObject.cpp:23-68) for a pair of vectors: over the common words in
 * ascending id, s += fabs(vi - wi) - fabs(vi) - fabs(wi) one rounded double operation at a time, then -s / 2.0 (the
 * lower_bound skips make the walk a merge).  Host code: no handle, no device.  Ids not strictly ascending: ORBX_ERR_ARG. */
int orbv_score_l1(const uint32_t *w1, const double *v1, int n1, const uint32_t *w2, const double *v2, int n2, double *out);
/* KeyFrameDatabase::KeyFrameDatabase (:33-37).  nwords = voc->size().  initial_entries: starting size of the entry pool in
 * (id, value) pairs, 0 = the default (2^20).  No usable GPU: ORBX_ERR_NO_DEVICE; there is no CPU path. */
int orbv_db_create(int nwords, int device, int initial_entries, orbv_db_t **out);
void orbv_db_destroy(orbv_db_t *db);
/* KeyFrameDatabase::add (:40-46).  n == 0 is legal (a keyframe no query can list).  Ids not strictly ascending or >= nwords,
 * or a kf_id that is in the database: ORBX_ERR_ARG.  The keyframe starts with an empty covisible list and mRelocScore 0.0f
 * (the reference leaves that member uninitialised, src/KeyFrame.cc:35: the value is this library's hypothesis). */
int orbv_db_add(orbv_db_t *db, int kf_id, const uint32_t *words, const double *values, int n);
/* KeyFrameDatabase::erase (:48-67); a kf_id that is not in the database: nothing happens, ORBX_OK.  With the keyframe go its
 * covisible list and its mRelocScore. */
int orbv_db_erase(orbv_db_t *db, int kf_id);
/* KeyFrameDatabase::clear (:69-73) */
int orbv_db_clear(orbv_db_t *db);
/* What pKFi->GetBestCovisibilityKeyFrames(10) returns (:151, :265), as ids in that order: the caller's graph.  n > 10, a
 * negative id, or a kf_id that is not in the database: ORBX_ERR_ARG.  An id the database does not hold at the time of a
 * query is skipped by it (such a keyframe's stamps can never equal the query's). */
int orbv_db_set_covisible(orbv_db_t *db, int kf_id, const int32_t *ids, int n);
/* keyframes in the database, (id, value) pairs they hold, capacity of the pool in pairs, device memory of the handle in bytes;
 * any pointer may be NULL */
int orbv_db_info(const orbv_db_t *db, int *keyframes, int64_t *entries, int64_t *pool_entries, size_t *device_bytes);
/* mpVoc->score(query, keyframe) as doubles for n keyframes of the database: the minScore loop of LoopClosing::DetectLoop
 * (src/LoopClosing.cc:135-147).  A kf_id that is not in the database: ORBX_ERR_ARG. */
int orbv_db_score(orbv_db_t *db, const uint32_t *qw, const double *qv, int nq, const int32_t *kf_ids, int n, double *scores);
/* KeyFrameDatabase::DetectLoopCandidates (:76-197).  connected = pKF->GetConnectedKeyFrames() as ids (ids the database does
 * not hold are ignored): they never enter the list.  maxCommonWords over the list, int minCommonWords = maxCommonWords*0.8f,
 * a listed keyframe is scored iff words > minCommonWords, enters lScoreAndMatch iff (float)score >= min_score; per entry
 * acc = best = si, then over its covisible list in order: a neighbour counts iff listed and scored by this query, acc += s2
 * in float, s2 > best makes it the best keyframe; bestAccScore starts at min_score; retained iff acc > 0.75f*bestAccScore;
 * cand = the best keyframes of the retained entries in list order, first occurrence only.  hits may be NULL.  A capacity too
 * small: ORBX_ERR_ARG with the needed counts in *ncand / *nhits (nhits may be NULL).  Empty query or nothing listed: ORBX_OK,
 * zero candidates. */
int orbv_db_detect_loop(orbv_db_t *db, const uint32_t *qw, const double *qv, int nq, const int32_t *connected, int nconnected,
                        float min_score, int32_t *cand, int cand_cap, int *ncand, orbv_db_hit_t *hits, int hit_cap, int *nhits);
/* KeyFrameDatabase::DetectRelocalizationCandidates (:199-309): no connected set and no min_score (every scored keyframe
 * enters lScoreAndMatch, bestAccScore starts at 0); a neighbour counts iff it is LISTED, and contributes its mRelocScore,
 * which only a relocalisation query that scores the keyframe writes - for a listed neighbour this query did not score it is
 * the value the last query that scored it left (0.0f if none did).  The scores are written before the capacities are
 * checked; repeating the query with larger buffers writes the same values again. */
int orbv_db_detect_reloc(orbv_db_t *db, const uint32_t *qw, const double *qv, int nq, int32_t *cand, int cand_cap, int *ncand,
                         orbv_db_hit_t *hits, int hit_cap, int *nhits);

/* ---- Optimizer::PoseOptimization(Frame *) (src/Optimizer.cc:239-451): the pose-only optimisation between the tracking
 * thread's two matcher calls (src/Tracking.cc:918, :1041, :1083, :1585-1616), on flat arrays.  One 6-DoF vertex, one unary
 * reprojection edge per valid entry (monocular when ur < 0, else stereo), 4 rounds of <= 10 Levenberg-Marquardt iterations with
 * the Huber kernel in the first three, classification by chi2 after every round; a restatement of the reference and the g2o
 * classes it drives, double with the reference's float narrowings.  The whole schedule is ONE kernel
 * launch, one workgroup per problem; two calls on the same input give the same bytes.  A singular normal matrix (fewer than
 * 3 active edges in a later round, coincident points) is not pinned to the reference: the call terminates, returns ORBX_OK
 * and its output is finite or unchanged.
 *
 * outlier[n] in/out = mvbOutlier: entries with valid == 0 keep the caller's value, the others get the last round's flag.
 * *ngood = nInitialCorrespondences - nBad; fewer than 3 correspondences: *ngood = 0, Tcw_out = Tcw_in, the valid entries' flags
 * cleared.  Tcw is the row-major float 4x4.  info (may be NULL): t / q the final estimate in double (q = x y z w),
 * iterations[r] / trials[r] the LM iterations and linear solves of round r, rounds the number of rounds run.
 * NULL pointers, n < 0, B < 0, offsets that start below 0 or decrease: ORBX_ERR_ARG, checked before the device is touched.
 * No usable GPU: ORBX_ERR_NO_DEVICE; there is no CPU path.  Scratch, pinned mirror and stream are per host thread
 * (orbx_thread_release_scratch). */
typedef struct { int32_t valid; float u, v, ur; float inv_sigma2; float wx, wy, wz; } orbo_observation_t; /* 32 B; ur < 0: monocular */
typedef struct { int32_t correspondences, bad; int32_t iterations[4], trials[4], rounds; double t[3], q[4]; } orbo_pose_info_t;
int orbo_pose_optimization(const orbo_observation_t *obs, int n, const orbm_camera_t *cam, const float *Tcw_in16,
                           float *Tcw_out16, uint8_t *outlier, int *ngood, orbo_pose_info_t *info /* may be NULL */, int device);
/* B independent problems in one launch (Relocalization's candidate keyframes): offsets[B+1] into obs / outlier, cams[B],
 * Tcw_in16 / Tcw_out16 [B][16], ngood[B], infos[B] (may be NULL).  Each problem's results are those of its single call. */
int orbo_pose_optimization_batch(const orbo_observation_t *obs, const int32_t *offsets, int B, const orbm_camera_t *cams,
                                 const float *Tcw_in16, float *Tcw_out16, uint8_t *outlier, int32_t *ngood,
                                 orbo_pose_info_t *infos, int device);
/* The frame left in HBM by extraction (see orbm_search_by_projection_frame_device): d_kun / d_uright are device arrays of n
 * entries, the observation of entry i is (d_kun[i].x, d_kun[i].y, d_uright[i]) with inv_level_sigma2[d_kun[i].octave]
 * (nlevels <= 16 host floats); only the 16-byte map-point records cross the bus.  Runs on `stream`; returns when the results
 * are on the host.  Same results as orbo_pose_optimization on the downloaded arrays. */
typedef struct { int32_t valid; float wx, wy, wz; } orbo_worldpos_t;
int orbo_pose_optimization_device(const orbx_keypoint_t *d_kun, const float *d_uright, int n, const float *inv_level_sigma2,
                                  int nlevels, const orbo_worldpos_t *pts, const orbm_camera_t *cam, const float *Tcw_in16,
                                  float *Tcw_out16, uint8_t *outlier, int *ngood, orbo_pose_info_t *info, int device, void *stream);

/* ---- Optimizer::OptimizeSim3 (src/Optimizer.cc:1051-1246): the refinement of a loop candidate's Sim3 between SearchBySim3 and
 * the projection search of LoopClosing::ComputeSim3 (src/LoopClosing.cc:336), on flat arrays.  One free 7-DoF vertex
 * (VertexSim3Expmap), per match the two edges EdgeSim3ProjectXYZ (point 2 through S12 into camera 1) and
 * EdgeInverseSim3ProjectXYZ (point 1 through S12^-1 into camera 2) with every map-point vertex fixed, the dense solver: a 7x7
 * Levenberg-Marquardt with the Huber kernel (delta = (float)sqrt(th2)) and g2o's NUMERIC Jacobian (central differences, 1e-9:
 * base_binary_edge.hpp:131-205; the analytic one is commented out in types_seven_dof_expmap).  optimize(5), the matches whose
 * last evaluation exceeded th2 on either edge dropped, optimize(10 if any was dropped, else 5) continuing from the first, the
 * same test again.  A restatement in double with the reference's float narrowings; the whole schedule is
 * ONE kernel launch, one workgroup per problem; two calls on the same input give the same bytes.  A singular normal matrix is
 * not pinned to the reference: the call terminates, returns ORBX_OK and its output is finite or unchanged.
 *
 * A row is one match the caller's filter accepted (:1106-1141: both map points present and not bad, the second observed in
 * keyframe 2): the two WORLD positions, the two undistorted keypoints (u1 v1 in keyframe 1, u2 v2 in keyframe 2) and
 * mvInvLevelSigma2[octave] of each.  The kernel moves the points into their camera frames in float as the reference's cv::Mat
 * product does (Tcw1, Tcw2: row-major float 4x4).  K = fx fy cx cy.  s, R, t: Sim3Solver's float estimate, from which the start
 * is g2o::Sim3(Matrix3d R, t, s) - Quaterniond(R) of the widened floats, not normalised.
 * dropped[i] = 1 for a match nulled in either round.  *ninliers = the reference's return value.  When fewer than 10 matches
 * survive the first round (or n < 10) the reference returns 0 with the first round's drops applied and the Sim3 as it came in:
 * then *ninliers = 0, info->rounds < 2 and the outputs hold the INPUT Sim3.  S12_out16 = Converter::toCvMat(Sim3): s*R | t as a
 * row-major float 4x4; info (may be NULL): the same estimate in double (q = x y z w), iterations[r] / trials[r] the LM
 * iterations and linear solves of round r.
 * NULL pointers, n < 0, B < 0, offsets that start below 0 or decrease, an inv_sigma2 or th2 that is negative or not finite:
 * ORBX_ERR_ARG, checked before the device is touched.  No usable GPU: ORBX_ERR_NO_DEVICE; there is no CPU path.  Scratch, pinned
 * mirror and stream are per host thread (orbx_thread_release_scratch).  (Prefix orbz_: orbo_ is PoseOptimization's section.) */
typedef struct { float w1[3], w2[3]; float u1, v1, u2, v2; float inv_sigma2_1, inv_sigma2_2; } orbz_sim3_match_t;   /* 48 B */
typedef struct { float Tcw1[16], Tcw2[16]; float K1[4], K2[4]; float s, R[9], t[3]; float th2; int32_t fix_scale; } orbz_sim3_problem_t; /* 220 B */
typedef struct { int32_t correspondences, bad, rounds, iterations[2], trials[2], reserved; double q[4], t[3], s; } orbz_sim3_info_t; /* 96 B */
int orbz_optimize_sim3(const orbz_sim3_match_t *m, int n, const orbz_sim3_problem_t *p, float *S12_out16, uint8_t *dropped,
                       int *ninliers, orbz_sim3_info_t *info /* may be NULL */, int device);
/* B independent problems (loop candidates) in one launch: offsets[B+1] into m / dropped (offsets[0] need not be 0), ps[B],
 * S12_out16 [B][16], ninliers[B], infos[B] (may be NULL).  Each problem's results are those of its single call, byte for byte. */
int orbz_optimize_sim3_batch(const orbz_sim3_match_t *m, const int32_t *offsets, int B, const orbz_sim3_problem_t *ps,
                             float *S12_out16, uint8_t *dropped, int32_t *ninliers, orbz_sim3_info_t *infos, int device);

/* ---- Initializer::Initialize (src/Initializer.cc:44-929): the monocular map initialisation Tracking runs on the matches of
 * ORBmatcher::SearchForInitialization (src/Tracking.cc:723, :757), on flat arrays.  2 x iterations RANSAC hypotheses (a
 * homography and a fundamental matrix from the 8 matches each set names), scored over all N matches; the choice RH > 0.40;
 * the decomposition into 8 (H) or 4 (F) motions, each checked by triangulating every inlier; the reference's acceptance rule.
 * A chain of four launches on one stream, every branch taken on the device, one synchronisation.  A
 * restatement in float with the reference's double promotions; the SVDs are this library's own Jacobi (csrc/orbx_jacobi_svd.h),
 * not OpenCV's.  Score sums run in match order: two calls give the same bytes, and a hypothesis' score depends on its model only.
 *
 * keys1 / keys2: x y pairs of ALL undistorted keypoints of the two frames (Normalize reads them all); matches [N][2]: indices
 * into keys1 / keys2 (mvMatches12); sets [iterations][8]: indices into matches (mvSets).  K4 = fx fy cx cy.
 * Returns ORBX_OK and *result = 1 / 0 (Initialize's bool).  On 0: R21, t21, P3D and triangulated are zero.  P3D [N][3] and
 * triangulated [N] are in MATCH order.  N < 8, iterations <= 0, an index out of range, NULL pointers, sigma that is not > 0:
 * ORBX_ERR_ARG, checked before the device is touched.  No usable GPU: ORBX_ERR_NO_DEVICE; there is no CPU path.  Scratch,
 * pinned mirror and stream are per host thread (orbx_thread_release_scratch). */
typedef struct {
    float SH, SF, RH;
    int32_t model;                     /* 0: homography, 1: fundamental (RH > 0.40 chooses 0) */
    int32_t best_iteration[2];         /* H, F: the first iteration whose score exceeds all before it; -1: none scored above 0 */
    int32_t inliers[2];                /* H, F */
    int32_t best_good, second_good;    /* the acceptance rule's counts (F: maxGood and the runner-up) */
    float parallax;                    /* of the best motion, degrees */
    int32_t ncand;                     /* motions checked: 8, 4, or 0 when the decomposition returned early */
    int32_t ngood[8];
    float cand_parallax[8];
    float H21[9], F21[9];              /* zero when best_iteration is -1 */
} orbi_init_info_t;
int orbi_initialize(const float *keys1, int n1, const float *keys2, int n2, const int32_t *matches, int N, const int32_t *sets,
                    int iterations, const float *K4, float sigma, float min_parallax, int min_triangulated, int *result,
                    float *R21, float *t21, float *P3D, uint8_t *triangulated, orbi_init_info_t *info /* may be NULL */, int device);
/* The two frames left in HBM by extraction: d_keys1 / d_keys2 are device arrays of n1 / n2 keypoint records (mvKeysUn); matches
 * and sets are on the host.  Runs on `stream`; returns when the results are on the host.  Same results as orbi_initialize. */
int orbi_initialize_device(const orbx_keypoint_t *d_keys1, int n1, const orbx_keypoint_t *d_keys2, int n2, const int32_t *matches,
                           int N, const int32_t *sets, int iterations, const float *K4, float sigma, float min_parallax,
                           int min_triangulated, int *result, float *R21, float *t21, float *P3D, uint8_t *triangulated,
                           orbi_init_info_t *info, int device, void *stream);
/* FindHomography and FindFundamental only: scores [2][iterations] (H first), inliersH / inliersF [N] of the best hypotheses (all
 * zero when none scored above 0); info->SH .. inliers, H21 and F21 are filled, the rest of info is zero. */
int orbi_search(const float *keys1, int n1, const float *keys2, int n2, const int32_t *matches, int N, const int32_t *sets,
                int iterations, float sigma, float *scores, uint8_t *inliersH, uint8_t *inliersF, orbi_init_info_t *info, int device);

/* ---- Sim3Solver (src/Sim3Solver.cc:37-423): the similarity transform LoopClosing::ComputeSim3 (src/LoopClosing.cc:248-339) looks
 * for between the current keyframe and each loop candidate, on flat arrays.  Per problem (candidate): up to `iterations` RANSAC
 * hypotheses, each Horn's closed form on the 3 pairs its set names followed by the two-way reprojection test over all pairs;
 * then the replay of the reference's sequential loop over the inlier counts.  A chain of three launches on one stream for ALL
 * problems of a call, one synchronisation.  A restatement in float with the reference's double promotions;
 * cv::eigen and cv::Rodrigues are this library's own (csrc/orbx_jacobi_eig.h), not OpenCV's.  Counts are integer: two calls give
 * the same bytes.
 *
 * pairs [n]: the world positions of the two matched map points and mvLevelSigma2[octave] of their keypoints.  A pair's
 * thresholds are (size_t)(9.210 * sigma2), TRUNCATED to an integer as the reference's std::vector<size_t> does.
 * sets [iterations][3]: indices into pairs, three different ones per set.  counts [iterations]; models [iterations][13]: s, R
 * row-major, t (may be NULL); flags [iterations][n] (may be NULL); hit_inliers [n]: the flags of the hit iteration, zero
 * without a hit.  hit_iteration: the first iteration whose count is > min_inliers, or -1; best_iteration: the LAST iteration
 * of the maximal count among those run (up to and including the hit, or all), -1 when iterations is 0; s, R, t, T12: its model.
 * iterations == 0 (what orbs_sim3_iterations answers for n < min_inliers) launches nothing and answers "no hit".
 * flags and hit_inliers have one entry per PAIR, that is per correspondence the caller's filter accepted (src/Sim3Solver.cc:62-103:
 * both points present and not bad, GetIndexInKeyFrame >= 0 in both keyframes, sigma2 from the keypoints at THOSE indices); the
 * reference's vbInliers has one entry per slot of vpMatched12, so the caller scatters them through its mvnIndices1 and a slot its
 * filter dropped stays false.  Only the inliers' matches go on into SearchBySim3 (src/LoopClosing.cc:323-328).
 * NULL pointers, iterations < 0, n < 0, n < 3 with iterations > 0, a set index out of range or a set naming a pair twice,
 * decreasing or negative offsets, a sigma2 that is negative or not finite: ORBX_ERR_ARG, checked before the device is touched.
 * No usable GPU: ORBX_ERR_NO_DEVICE; there is no CPU path.  Scratch, pinned mirror and stream are per host thread
 * (orbx_thread_release_scratch). */
typedef struct { float w1[3], w2[3]; float sigma2_1, sigma2_2; } orbs_pair_t;                         /* 32 B */
typedef struct { float Tcw1[16], Tcw2[16]; float K1[4], K2[4]; int32_t fix_scale, min_inliers; } orbs_problem_t;   /* K: fx fy cx cy */
typedef struct { int32_t n, iterations, hit_iteration, best_iteration, best_inliers; float s, R[9], t[3], T12[16]; } orbs_sim3_info_t;
/* Host code, no device: what SetRansacParameters (:114-138) leaves in mRansacMaxIts; 0 when n < min_inliers (iterate answers
 * bNoMore without looking, :146-150). */
int orbs_sim3_iterations(int n, double probability, int min_inliers, int max_iterations);
int orbs_sim3_ransac(const orbs_pair_t *pairs, int n, const orbs_problem_t *problem, const int32_t *sets, int iterations,
                     int32_t *counts, float *models, uint8_t *flags, uint8_t *hit_inliers, orbs_sim3_info_t *info, int device);
/* B problems in one chain of launches: problem b owns pairs offsets[b] .. offsets[b+1]-1 and sets set_offsets[b] ..
 * set_offsets[b+1]-1 (its sets index ITS pairs from 0).  counts [set_offsets[B]], models [set_offsets[B]][13], flags: problem
 * b's [iterations_b][n_b] block after those of the problems before it, hit_inliers [offsets[B]], infos [B].  Each problem's
 * results are those of its single call.  An empty problem is allowed and answers "no hit".
 * offsets[0] and set_offsets[0] need not be 0 (a caller may pass offsets + k, set_offsets + k, problems + k, B - k to run the
 * problems from k on, with the arrays' base pointers unchanged): whatever is indexed by a pair or by a set - pairs, sets,
 * counts, models, hit_inliers - is read and written at the positions the offsets name, and nothing before offsets[0] /
 * set_offsets[0] is touched; flags and infos are counted from the call's own first problem (flags[0], infos[0]). */
int orbs_sim3_ransac_batch(const orbs_pair_t *pairs, const int32_t *offsets, int B, const orbs_problem_t *problems,
                           const int32_t *sets, const int32_t *set_offsets, int32_t *counts, float *models, uint8_t *flags,
                           uint8_t *hit_inliers, orbs_sim3_info_t *infos, int device);

/* ---- PnPsolver (src/PnPsolver.cc:67-950): the EPnP RANSAC Tracking::Relocalization (src/Tracking.cc:1530-1556) runs for every
 * candidate keyframe, on flat arrays.  One call covers the iterations ONE PnPsolver::iterate call may run, for B problems
 * (candidates): per set EPnP on the 4 correspondences it names and the reprojection test over all n (k_pnp_ransac); EPnP again on
 * the inlier set of every iteration that becomes the best one, and on the prior best set the caller carries (k_pnp_refine); then
 * the replay of the reference's sequential loop (k_pnp_select).  Three launches on one stream for ALL problems, one
 * synchronisation.  EPnP is in double as in the reference; the five OpenCV calls it makes are this
 * library's own Jacobi routines (csrc/orbx_jacobi_eig.h, csrc/orbx_jacobi_svd.h), not OpenCV's.  Counts are integer: two calls
 * give the same bytes.
 *
 * corrs [n]: the world position of the map point, the undistorted keypoint, mvLevelSigma2[octave]; a correspondence's threshold
 * is sigma2 * th2 in float.  problem: K = fx fy cx cy; min_inliers and max_iterations as orbp_pnp_parameters adjusts them;
 * iterations_done = mnIterations before the call; prior_best_inliers = mnBestInliers, and prior_best_flags [n] = mvbBestInliers
 * (NULL when the prior count is 0).  sets [iterations][4]: indices into corrs, four different ones per set.
 * Per iteration: counts; models [iterations][12] double (R row-major, t; may be NULL); tcws [iterations][16] float (may be NULL);
 * choices [iterations]: which beta approximation (1-3) gave the least reprojection error (may be NULL); flags [iterations][n]
 * (may be NULL).  Per refinement slot (slot i < iterations: iteration i's own flags; slot `iterations`: the prior best set):
 * refined_counts [iterations + 1], -1 where the slot is no record and nothing was computed (may be NULL).
 * inliers [n]: the flags that go with the returned pose; best_flags [n]: mvbBestInliers after the call, to be passed back.
 * info: hit_iteration (the iteration at which a refinement counted > min_inliers) or -1; iterations_run; best_iteration or -1
 * when the prior best still stands; best_inliers; refined_inliers (at a hit); no_more; pose: ORBP_POSE_NONE, ORBP_POSE_REFINED
 * (Tcw = mRefinedTcw), ORBP_POSE_BEST (exhausted, Tcw = this call's best iteration's) or ORBP_POSE_PRIOR_BEST (exhausted and the
 * prior best stands: the caller returns the mBestTcw it kept); best_Tcw: this call's best iteration's pose (zero without one).
 * A problem with n < min_inliers or without sets launches nothing and answers no_more (:173-177).
 * NULL pointers, negative sizes, sets for a problem with n < 4 or n < min_inliers, a set index out of range or a set naming a
 * correspondence twice, decreasing or negative offsets, a sigma2 that is negative or not finite, a prior count that is not
 * the number of prior flags set: ORBX_ERR_ARG, checked before the device is touched.  No usable GPU: ORBX_ERR_NO_DEVICE; there is
 * no CPU path.  Scratch, pinned mirror and stream are per host thread (orbx_thread_release_scratch). */
typedef struct { float w[3]; float u, v; float sigma2; } orbp_corr_t;                                   /* 24 B */
typedef struct { float K[4]; float th2; int32_t min_inliers, max_iterations, iterations_done, prior_best_inliers; } orbp_problem_t;   /* 36 B */
#define ORBP_POSE_NONE 0
#define ORBP_POSE_REFINED 1
#define ORBP_POSE_BEST 2
#define ORBP_POSE_PRIOR_BEST 3
typedef struct { int32_t n, iterations, hit_iteration, iterations_run, best_iteration, best_inliers, refined_inliers, no_more, pose;
                 float Tcw[16], best_Tcw[16]; } orbp_pnp_info_t;                                       /* 164 B */
/* Host code, no device: SetRansacParameters (:121-157).  adj_min_inliers = max(int(n * epsilon), min_inliers, min_set);
 * adj_max_iterations = max(1, min(nIterations, max_iterations)).  min_set != 4, n < 0 or a NULL result: ORBX_ERR_ARG. */
int orbp_pnp_parameters(int n, double probability, int min_inliers, int max_iterations, int min_set, float epsilon,
                        int *adj_min_inliers, int *adj_max_iterations);
int orbp_pnp_ransac(const orbp_corr_t *corrs, int n, const orbp_problem_t *problem, const int32_t *sets, int iterations,
                    const uint8_t *prior_best_flags, int32_t *counts, double *models, float *tcws, int32_t *choices, uint8_t *flags,
                    int32_t *refined_counts, uint8_t *inliers, uint8_t *best_flags, orbp_pnp_info_t *info, int device);
/* B problems in one chain of launches, laid out as orbs_sim3_ransac_batch lays them out: corrs, prior_best_flags, inliers and
 * best_flags [offsets[B]]; counts, models, tcws, choices [set_offsets[B]]; refined_counts: problem b's iterations_b + 1 slots
 * start at set_offsets[b] + b; flags: problem b's [iterations_b][n_b] block after those of the problems before it.
 * offsets[0] and set_offsets[0] need not be 0, as there: corrs, prior_best_flags, sets, counts, models, tcws, choices, inliers
 * and best_flags are read and written at the positions the offsets name and nothing before them is touched; flags and infos
 * start at flags[0] and infos[0]; and in refined_counts' set_offsets[b] + b the b is counted in THIS call, so the
 * set_offsets[B] - set_offsets[0] + B slots written start at set_offsets[0]. */
int orbp_pnp_ransac_batch(const orbp_corr_t *corrs, const int32_t *offsets, int B, const orbp_problem_t *problems,
                          const int32_t *sets, const int32_t *set_offsets, const uint8_t *prior_best_flags, int32_t *counts,
                          double *models, float *tcws, int32_t *choices, uint8_t *flags, int32_t *refined_counts, uint8_t *inliers,
                          uint8_t *best_flags, orbp_pnp_info_t *infos, int device);

/* ---- LocalMapping::CreateNewMapPoints (reference: src/LocalMapping.cc:215-460; prefix orbl_) ------------------------------------
 * What happens to the pairs ORBmatcher::SearchForTriangulation returns: per matched pair the ray-parallax test, a 4x4 SVD
 * (orbi_initialize's Jacobi SVD, not pinned to OpenCV's) or KeyFrame::UnprojectStereo, two depth tests, two chi-square reprojection
 * tests and the scale-consistency test, one thread per match, :299-439 statement by statement ("k_new_points").
 * A keyframe is its view, its undistorted keypoints mvKeysUn (orbx_keypoint_t, as the matchers take them), an optional stereo array
 * (NULL: a monocular keyframe; ur < 0: a monocular feature; raw_u / raw_v: mvKeys, which UnprojectStereo reads) and its level
 * tables mvScaleFactors / mvLevelSigma2 [view.nlevels].
 * Status of a row, in the reference's order: 0 accepted (triangulated), 1 accepted from UnprojectStereo of keyframe 1, 2 of keyframe
 * 2, -1 low parallax, -2 w == 0, -3 z1 <= 0, -4 z2 <= 0, -5 reprojection in keyframe 1, -6 in keyframe 2, -7 a zero distance,
 * -8 scale ratio, -9 the pair of keyframes was skipped by the baseline rule, -10 no match (orbl_create_new_map_points only).
 * x y z hold x3D whenever it was formed (0, 1, 2, -3 .. -8) and are zero otherwise; cos_stereo = min(cosParallaxStereo1, 2); rows
 * of status -9 / -10 are all zero but the status.
 * ORBX_ERR_ARG, checked before the device is touched, with every output zeroed: a NULL pointer, a NaN in a view, nlevels outside
 * 1..ORBL_MAX_LEVELS, a level sigma2 or scale factor that is not positive, a keypoint that is NaN or whose octave is outside
 * [0, nlevels), a stereo feature (ur >= 0) whose depth is not positive (the reference dereferences an empty matrix there) or whose
 * raw position is NaN, a match index outside [0, n).  No usable GPU: ORBX_ERR_NO_DEVICE; there is no CPU path.  Scratch, pinned
 * mirror and stream are per host thread (orbx_thread_release_scratch). */
#define ORBL_MAX_LEVELS 16
#define ORBL_MAX_NEIGHBOURS 32
typedef struct { float Tcw[16]; float Ow[3]; float fx, fy, cx, cy, invfx, invfy, mb, mbf, scale_factor; int32_t nlevels; } orbl_view_t;   /* 116 B; Tcw row-major, Ow as KeyFrame::SetPose stores it (-Rwc*tcw) */
typedef struct { float ur, depth, raw_u, raw_v; } orbl_stereo_t;                                                                          /* 16 B */
typedef struct { float x, y, z; int32_t status; float cos_rays, cos_stereo; int32_t reserved[2]; } orbl_point_t;                          /* 32 B */
typedef struct { const orbl_view_t *view; const orbx_keypoint_t *kp; const orbl_stereo_t *st /* may be NULL */; int32_t n;
                 const float *scale_factors, *level_sigma2; } orbl_keyframe_t;
/* One pair of keyframes, one launch: pairs [nm][2] = (idx1, idx2), points [nm], *nnew = rows with status >= 0.  nm == 0: ORBX_OK,
 * no launch. */
int orbl_triangulate(const orbl_view_t *view1, const orbx_keypoint_t *kp1, const orbl_stereo_t *st1, int n1, const float *scale_factors1,
                     const float *level_sigma2_1, const orbl_view_t *view2, const orbx_keypoint_t *kp2, const orbl_stereo_t *st2, int n2,
                     const float *scale_factors2, const float *level_sigma2_2, const int32_t *pairs, int nm, orbl_point_t *points,
                     int *nnew, int device);
/* npairs pairs of keyframes (kf1[p], kf2[p]) in one launch: pair p's matches are pairs[match_off[p] .. match_off[p + 1]) and its rows
 * points[the same]; match_off[0] == 0, an empty pair is legal; nnew [npairs]. */
int orbl_triangulate_batch(const orbl_keyframe_t *kf1, const orbl_keyframe_t *kf2, int npairs, const int32_t *match_off,
                           const int32_t *pairs, orbl_point_t *points, int32_t *nnew, int device);
/* The baseline rule of :252-269, host code: 1 = go on, 0 = skip the neighbour.  baseline = (float)norm(Ow2 - Ow1); stereo / RGB-D:
 * skip when baseline < view2->mb; monocular: skip when (double)(baseline / median_depth2) < 0.01.  NULL view: ORBX_ERR_ARG. */
int orbl_baseline_ok(const orbl_view_t *view1, const orbl_view_t *view2, int monocular, float median_depth2);
/* LocalMapping::ComputeF12 with SkewSymmetricMatrix (:544-561, :706-711), host code: every cv::Mat product materialised to float in
 * the order written (csrc/orbx_cvmath.h).  K = fx fy cx cy.  Not pinned to an OpenCV build. */
int orbl_compute_f12(const float *Tcw1_16, const float *K1_4, const float *Tcw2_16, const float *K2_4, float *F12_9);
/* CreateNewMapPoints' loop over the covisible neighbours (:245-459) as ONE stream-ordered submission.  cur: the current keyframe, nq =
 * cur->n features with descriptors q_desc [nq][32] and q_flags [nq] as orbm_search_for_triangulation takes them (bit 0: a query, i.e. no
 * map point yet; bit 1: stereo).  A neighbour is the candidate side of orbm_search_for_triangulation (kf.kp = kp2, kf.n = nc, c_desc,
 * c_flags, the four node lists, F12, the epipole ex / ey; the matcher reads the NEIGHBOUR's level tables) with its view, stereo array
 * and, for the monocular rule, ComputeSceneMedianDepth(2).  Everything is staged once.  Then, for every neighbour that passes
 * orbl_baseline_ok, in order: the matcher's kernels on the device-resident flags, and k_new_points over all nq queries, which reads
 * match_q on the device, writes status -10 where there is no match and clears bit 0 of the device q_flags[idx1] for every accepted
 * row - the next neighbour's matcher no longer takes that feature as a query (src/ORBmatcher.cc:703-704).  One synchronisation at the end.
 * Outputs, neighbour i at [i * nq]: match_q [nn][nq], points [nn][nq]; nmatches, nnew, skipped [nn] (skipped: 1 = the baseline rule, its
 * rows have status -9 and match_q -1); q_flags_out [nq]: the flags after the last neighbour.  nn > ORBL_MAX_NEIGHBOURS, or more than
 * 4096 candidates in one vocabulary node of some neighbour: ORBX_ERR_UNSUPPORTED; on any error match_q is all -1, points, nmatches,
 * nnew and skipped are zero and q_flags_out is q_flags. */
typedef struct { orbl_keyframe_t kf; const uint8_t *c_desc, *c_flags; const int32_t *node_qstart, *q_items, *node_cstart, *c_items; int32_t nnodes;
                 float F12[9]; float ex, ey; float median_depth2; } orbl_neighbour_t;
int orbl_create_new_map_points(const orbl_keyframe_t *cur, const uint8_t *q_desc, const uint8_t *q_flags, const orbl_neighbour_t *neighbours, int nn,
                               int monocular, int max_dist, int check_orientation, int32_t *match_q, orbl_point_t *points, int32_t *nmatches,
                               int32_t *nnew, uint8_t *skipped, uint8_t *q_flags_out, int device);

/* ---- Optimizer::LocalBundleAdjustment (src/Optimizer.cc:453-780) and Optimizer::BundleAdjustment (:49-237; prefix orbb_) ----------
 * The bundle adjustment LocalMapping::Run calls after CreateNewMapPoints (src/LocalMapping.cc:89), on flat arrays: 6-DoF keyframe
 * vertices, 3-DoF map-point vertices (always marginalised, never fixed), one EdgeSE3ProjectXYZ (ur < 0) or EdgeStereoSE3ProjectXYZ
 * per observation, Levenberg-Marquardt with the Huber kernel over the Schur complement.  A restatement in double with the
 * reference's float narrowings ("k_lba_*").  The landmark block is block-diagonal and the reduced system, 6 Nf
 * square for Nf free keyframes, is DENSE here: it is meant for a local window (a few tens of free keyframes; it stays correct for
 * any Nf memory allows, one workgroup factorises it).  For a loop-closure-sized map: orbb_global_bundle_adjustment, below.
 * The host drives the iterations and trials: a handful of launches per linearisation and per trial on this thread's stream, one
 * stream synchronisation per trial, none device-wide.  Every sum has one owner and a fixed order: two calls give the same bytes.
 * Not pinned to g2o: the order of vertices and edges inside its sums, Eigen's sparse SimplicialLDLT against the dense LDL^T here,
 * Matrix3d::inverse, the device's sin / cos / sqrt; a zero, negative or non-finite pivot rejects the trial (tempChi = DBL_MAX).
 *
 * kfs [K]: Tcw row-major float 4x4, fx fy cx cy, bf = mbf, fixed != 0 for every "fixed camera" of :489-504 and for a local keyframe
 * with mnId == 0.  pts [P]: world positions.  obs [E] in any order: keyframe kf observes point pt at the undistorted keypoint (u, v),
 * ur = mvuRight (< 0: a monocular observation), inv_sigma2 = mvInvLevelSigma2[octave]; a keyframe observes a point at most once.
 * stop (may be NULL) is pbStopFlag, polled exactly where the reference reads it: at :655 (set: the call returns with the inputs
 * as outputs and nothing erased), before every iteration, after a rejected trial when another would follow, and at :664 (set: no
 * classification and no second round; the final classification and the outputs still happen).
 * Tcw_out16 [K][16]: Converter::toCvMat of the estimates, a fixed keyframe's byte for byte as it came in; pts_out3 [P][3];
 * erase [E]: 1 where the final check (chi2 of the edge's LAST evaluation > 5.991 / 7.815, or a depth that is not positive at the
 * final estimates) asks for EraseMapPointMatch / EraseObservation.  info, kf_est7 [K][7] (q = x y z w, then t) and pt_est3 [P][3]
 * (the double estimates) may be NULL.  K, P or E may be 0.
 * NULL pointers, negative sizes, an index out of range, a (kf, pt) pair that occurs twice, an input that is NaN or infinite, a
 * negative inv_sigma2, a schedule outside its ranges: ORBX_ERR_ARG, checked before the device is touched.  No usable GPU:
 * ORBX_ERR_NO_DEVICE; there is no CPU path.  Scratch, pinned mirror and stream are per host thread (orbx_thread_release_scratch). */
#define ORBB_MAX_ITERATIONS 100   /* per round */
#define ORBB_STOP_BEFORE 1        /* info->stopped_at: where stop first answered non-zero; 0: it never did.  1: at :655 */
#define ORBB_STOP_ROUND1 2        /* inside the first optimize() */
#define ORBB_STOP_BETWEEN 3       /* at :664 */
#define ORBB_STOP_ROUND2 4        /* inside the second optimize() */
typedef struct { float Tcw[16]; float fx, fy, cx, cy, bf; int32_t fixed; } orbb_keyframe_t;       /* 88 B */
typedef struct { float x, y, z; } orbb_point_t;                                                   /* 12 B */
typedef struct { int32_t kf, pt; float u, v, ur, inv_sigma2; } orbb_observation_t;                /* 24 B */
/* rounds: 1 or 2 optimize() calls of iterations[r] each, with (robust[r] != 0) or without the Huber kernel of the two deltas; two
 * rounds have the :664 read of the flag and the classification (chi2 > 5.991 / 7.815 or depth not positive -> level 1) between
 * them; classify: the final check fills erase; check_stop_first: the :655 read. */
typedef struct { int32_t rounds, iterations[2], robust[2]; float delta_mono, delta_stereo; int32_t classify, check_stop_first; } orbb_schedule_t;   /* 36 B */
/* free_poses[r]: keyframes optimised in round r (not fixed, with an edge at level 0); stop_poll: the number of the poll counted in
 * stopped_at, from 1; polls: how often stop was called */
typedef struct { int32_t rounds, iterations[2], trials[2], free_poses[2], stopped_at, stop_poll, polls, erased; } orbb_info_t;     /* 44 B */
int orbb_optimize(const orbb_keyframe_t *kfs, int K, const orbb_point_t *pts, int P, const orbb_observation_t *obs, int E,
                  const orbb_schedule_t *schedule, int (*stop)(void *), void *stop_user, float *Tcw_out16, float *pts_out3,
                  uint8_t *erase, orbb_info_t *info, double *kf_est7, double *pt_est3, int device);
/* The schedule of :569-570, :655-707: {2, {5, 10}, {1, 0}, (float)sqrt(5.991), (float)sqrt(7.815), 1, 1} */
int orbb_local_bundle_adjustment(const orbb_keyframe_t *kfs, int K, const orbb_point_t *pts, int P, const orbb_observation_t *obs, int E,
                                 int (*stop)(void *), void *stop_user, float *Tcw_out16, float *pts_out3, uint8_t *erase,
                                 orbb_info_t *info, double *kf_est7, double *pt_est3, int device);
/* Optimizer::BundleAdjustment over the same kernels: one optimize(iterations), the Huber kernel iff robust, no classification, no
 * :655 read; its monocular delta is (float)sqrt(5.99), not 5.991 (:85).  The caller leaves out bad keyframes and points and the
 * points without an observation (:175-179), and sets fixed for mnId == 0.  What CreateInitialMapMonocular's
 * GlobalBundleAdjustemnt(mpMap, 20) needs (src/Tracking.cc:700). */
int orbb_bundle_adjustment(const orbb_keyframe_t *kfs, int K, const orbb_point_t *pts, int P, const orbb_observation_t *obs, int E,
                           int iterations, int robust, int (*stop)(void *), void *stop_user, float *Tcw_out16, float *pts_out3,
                           orbb_info_t *info, double *kf_est7, double *pt_est3, int device);
/* The BLOCKED reduced-system path, for a loop-closure-sized map (LoopClosing::RunGlobalBundleAdjustment's
 * GlobalBundleAdjustemnt(mpMap, 10, &mbStopGBA, nLoopKF, false), src/LoopClosing.cc:659): the same edges, Jacobians, Schur
 * complement and Levenberg-Marquardt, but the Schur complement is summed from the pairs of keyframes that do co-observe a point
 * (per round the host builds the block pattern and each block's contributions; no [Nf][P] table), and the dense LDL^T is blocked
 * over the whole GPU in panels of 8 poses: factorise the diagonal block, solve the rows below it, update the trailing lower
 * triangle tile by tile; the substitutions are blocked the same way.  Every entry of the factor and of the solution receives the
 * operations of the one-workgroup factorisation in the same order, so one thread per workgroup gives the same bytes on both
 * paths; the matrix is still dense (n^2 doubles, n = 6 Nf).  The functions above keep their path: nothing switches by size.
 * binfo (may be NULL), per round: blocks of the pattern (the diagonal ones included), panels = ceil(Nf / 8), contributions summed
 * over the blocks; launches: kernel launches of the call.  Arguments, errors and scratch as for orbb_optimize. */
typedef struct { int32_t blocks[2], panels[2]; int64_t contributions[2], launches; } orbb_blocked_info_t;   /* per round; 40 B */
int orbb_optimize_blocked(const orbb_keyframe_t *kfs, int K, const orbb_point_t *pts, int P, const orbb_observation_t *obs, int E,
                          const orbb_schedule_t *schedule, int (*stop)(void *), void *stop_user, float *Tcw_out16, float *pts_out3,
                          uint8_t *erase, orbb_info_t *info, double *kf_est7, double *pt_est3, orbb_blocked_info_t *binfo, int device);
/* orbb_bundle_adjustment's schedule on the blocked path: one optimize(iterations), the Huber kernel iff robust, the monocular
 * delta (float)sqrt(5.99), no classification and no :655 read.  The caller writes mTcwGBA / mPosGBA from the outputs. */
int orbb_global_bundle_adjustment(const orbb_keyframe_t *kfs, int K, const orbb_point_t *pts, int P, const orbb_observation_t *obs, int E,
                                  int iterations, int robust, int (*stop)(void *), void *stop_user, float *Tcw_out16, float *pts_out3,
                                  orbb_info_t *info, double *kf_est7, double *pt_est3, orbb_blocked_info_t *binfo, int device);

/* ---- Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:783-1049; prefix orbg_) ----------------------------------------------------
 * The pose graph LoopClosing::CorrectLoop optimises after it has fused the loop (src/LoopClosing.cc:576), on flat arrays: one
 * VertexSim3Expmap (7 unknowns) per keyframe, one EdgeSim3 (7 residuals, identity information, numeric Jacobians with delta = 1e-9)
 * per edge, no robust kernel, Levenberg-Marquardt from lambda = 1e-16 over the whole Hpp (no vertex is marginalised).  Double
 * throughout; DESIGN.md section 6, "k_eg_*".  The host computes the symbolic factorisation once per call (ordering, elimination
 * tree, block pattern with fill, the update list of every block); the device factorises by a left-looking block LDL^T without
 * pivoting, one launch per level of the elimination tree.  The host drives iterations and trials with one stream synchronisation per
 * trial.  Every sum has one owner and a fixed order: two calls give the same bytes.
 *
 * vertices [N]: Scw = the vScw entry (CorrectedSim3's, or Sim3(Rcw, tcw, 1) of the keyframe's pose widened), Snc with has_nc != 0 =
 * the NonCorrectedSim3 entry, fixed != 0 for pLoopKF.  Any number of vertices may be fixed, none included (the reference runs either
 * way); a vertex without an edge keeps its estimate.  edges [E]: vertex 0 of the EdgeSim3 is i, vertex 1 is j; kind 0 (a loop
 * connection, :854-882) measures Scw[j] * Scw[i]^-1, kind 1 (spanning tree, loop, covisibility, :885-985) takes Snc for an end whose
 * has_nc is set; a pair may occur any number of times.  points [P]: ref = the vertex of mnCorrectedReference or of the reference
 * keyframe (:1025-1034).  iterations: 0..ORBG_MAX_ITERATIONS (the reference: 20).
 * Tcw_out16 [N][16]: [R, t / s] of every estimate, a fixed vertex's too (:1001-1011); pts_out3 [P][3]: correctedSwr.map(Srw.map(P))
 * in double, narrowed (:1037-1045); est_out8 [N][8] (may be NULL): the estimates q (x y z w), t, s; info may be NULL.
 * NULL pointers, negative sizes, an index out of range, i == j, a value that is NaN or infinite, s <= 0, iterations outside its
 * range: ORBX_ERR_ARG before a device is touched.  Connectivity is not checked: a component that does not reach a fixed vertex
 * leaves a singular matrix that only lambda regularises, as in the reference.  Scratch per host thread (orbx_thread_release_scratch). */
#define ORBG_MAX_ITERATIONS 64
#define ORBG_END_ITERATIONS 0     /* info->end: every iteration asked for has run */
#define ORBG_END_QMAX 1           /* ten trials of one iteration were rejected */
#define ORBG_END_RHO0 2           /* a trial's rho was exactly 0 */
#define ORBG_END_SOLVER 3         /* as ORBG_END_QMAX or ORBG_END_RHO0, and the last trial's factorisation met a bad pivot */
#define ORBG_END_NBAD 4           /* three iterations in a row gained less than 1e-3 of their chi2: the reference's _nBad >= 3 (optimization_algorithm_levenberg.cpp:152-160) */
typedef struct { double q[4], t[3], s; } orbg_sim3_t;                                   /* 64 B; q = x y z w */
typedef struct { orbg_sim3_t Scw, Snc; int32_t has_nc, fixed; } orbg_vertex_t;          /* 136 B */
typedef struct { int32_t i, j, kind; } orbg_edge_t;                                     /* 12 B */
typedef struct { float x, y, z; int32_t ref; } orbg_point_t;                            /* 16 B */
/* trials: their total; trials_it[k]: of iteration k; free_vertices: columns (not fixed, with an edge); blocks: 7x7 blocks of the
 * factor, the diagonal ones included; levels: launch levels of the elimination tree; launches: kernel launches of the call */
typedef struct { int32_t iterations, trials, end, free_vertices, blocks, levels, launches, pad; double chi2_first, chi2_last;
                 int32_t trials_it[ORBG_MAX_ITERATIONS]; } orbg_info_t;                 /* 304 B */
int orbg_optimize_essential_graph(const orbg_vertex_t *vertices, int N, const orbg_edge_t *edges, int E, const orbg_point_t *points, int P,
                                  int fix_scale, int iterations, float *Tcw_out16, float *pts_out3, double *est_out8, orbg_info_t *info,
                                  int device);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Covisibility: KeyFrame::UpdateConnections (src/KeyFrame.cc:290-380), LocalMapping::KeyFrameCulling (src/LocalMapping.cc:640-704)
 * and MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:340-383) over ONE observation table, the reference's
 * std::map<KeyFrame*, size_t> of every map point laid out as rows.  DESIGN.md section 6, "k_cov_*".
 *
 * Keyframes are addressed by slot 0..K-1; slot order stands for the walk order of the reference's std::map<KeyFrame*, ...>, which is
 * pointer order there (the host classes fill slots in ascending mnId: a stated difference).  Point p owns
 * obs[obs_off[p] .. obs_off[p+1]), strictly ascending in kf.  Query q is keyframe slot query_kf[q] with the features
 * feat[feat_off[q] .. feat_off[q+1]) in feature-slot order: GetMapPointMatches().  scale_factors[nlevels] is the one extractor's table
 * every keyframe of the reference copies.
 *
 * PRECONDITION (not checked here; the Python wrappers check it by default): for a query keyframe, a feature that names point p
 * implies that p's list holds an observation by that keyframe, and for orbc_keyframe_culling an observation (kf, idx) of p by a query
 * keyframe implies that feature idx of that query names p (KeyFrame::SetBadFlag walks the features, src/KeyFrame.cc:470-472).  The
 * query keyframes of a culling call are distinct.
 *
 * Every index range is checked on the host in the pass that packs the upload: kf, ref_kf, point, octave < nlevels, idx >= 0, offsets
 * that start at 0 and do not decrease, kf strictly ascending inside a list, query_kf, a repeated culling query, th < 1, cap < 0:
 * ORBX_ERR_ARG with a message, before a device is touched.  More than ORBC_MAX_CULL_KEYFRAMES keyframes in a culling call:
 * ORBX_ERR_UNSUPPORTED.  No usable GPU: ORBX_ERR_NO_DEVICE; there is no CPU path.  Scratch, pinned mirror and stream are per host
 * thread (orbx_thread_release_scratch); a call is one upload, its launches, one download and one stream synchronisation. */
#define ORBC_LDS_KEYFRAMES 8192          /* k_cov_count keeps the counters of one query in LDS up to this K (32 KiB of the CU's 160); beyond: its row of a global block */
#define ORBC_SORT_LDS 1024               /* k_cov_order sorts a list up to this length in LDS; beyond: the radix core of orbx_cloud_dev.h */
#define ORBC_MAX_CULL_KEYFRAMES 262144   /* k_cull keeps the set of culled keyframes as one bit each in LDS (32 KiB) */
typedef struct { int32_t id;            /* mnId: 0 is never culled (src/LocalMapping.cc:651, src/KeyFrame.cc:458) */
                 uint8_t bad;           /* mbBad: carried, read by no kernel (src/KeyFrame.cc:310 tests the POINT, never the keyframe) */
                 uint8_t not_erase;     /* mbNotErase (src/KeyFrame.cc:460-464) */
                 uint8_t pad[2];
                 float Ow[3];           /* GetCameraCenter() (src/MapPoint.cc:362) */
                 float th_depth;        /* mThDepth (src/LocalMapping.cc:668) */
} orbc_keyframe_t;                      /* 24 B */
typedef struct { float pos[3];          /* mWorldPos (src/MapPoint.cc:357) */
                 int32_t ref_kf;        /* slot of mpRefKF, -1 for none (src/MapPoint.cc:356) */
                 uint8_t bad;           /* isBad() (src/KeyFrame.cc:310, src/LocalMapping.cc:664) */
                 uint8_t pad[3];
} orbc_point_t;                         /* 20 B */
typedef struct { int32_t kf;            /* slot: the map's key */
                 int32_t idx;           /* the map's value: the feature index in that keyframe */
                 uint8_t octave;        /* mvKeysUn[idx].octave (src/LocalMapping.cc:683, src/MapPoint.cc:373) */
                 uint8_t stereo;        /* mvuRight[idx] >= 0 (src/MapPoint.cc:121-127: nObs counts 2) */
                 uint8_t pad[2];
} orbc_observation_t;                   /* 12 B */
typedef struct { int32_t point;         /* -1: a NULL slot of mvpMapPoints */
                 int32_t octave;        /* mvKeysUn[i].octave (src/LocalMapping.cc:675) */
                 float depth;           /* mvDepth[i] (src/LocalMapping.cc:668) */
} orbc_feature_t;                       /* 12 B */
typedef struct { float normal[3];       /* mNormalVector (src/MapPoint.cc:381) */
                 float max_distance;    /* mfMaxDistance (src/MapPoint.cc:379) */
                 float min_distance;    /* mfMinDistance (src/MapPoint.cc:380) */
                 int32_t status;        /* ORBC_NORMAL_* ; nonzero: the five floats are 0 */
} orbc_normal_t;                        /* 24 B */
#define ORBC_NORMAL_OK 0
#define ORBC_NORMAL_BAD 1                /* the point is bad (src/MapPoint.cc:349) */
#define ORBC_NORMAL_NO_OBSERVATION 2     /* its list is empty (src/MapPoint.cc:359) */
#define ORBC_NORMAL_NO_REFERENCE 3       /* ref_kf is -1 or not in its list: the reference is undefined there (observations[pRefKF] inserts 0, :373) */
typedef struct { const orbc_keyframe_t *kf; int32_t K; const orbc_point_t *pts; int32_t P; const int32_t *obs_off /* [P + 1] */;
                 const orbc_observation_t *obs; const float *scale_factors; int32_t nlevels; } orbc_table_t;
typedef struct { const int32_t *query_kf; int32_t Q; const int32_t *feat_off /* [Q + 1] */; const orbc_feature_t *feat; } orbc_queries_t;
/* UpdateConnections of Q keyframes, each independent of the others.  counter[k] = the number of (feature, observation) pairs of the
 * query in which the feature's point is neither -1 nor bad and the observation's kf == k != the query's slot; a point named by two
 * features counts twice (:303-321).  Every counter 0: n[q] = 0 (:324-325).  Otherwise the list is every k with counter[k] >= th (the
 * reference: 15), or, if there is none, the one entry (nmax, the first slot in ascending order that reaches the strict maximum)
 * (:335-353); ordered by descending weight and, among equal weights, descending slot: sort on (weight, pointer) and push_front
 * (:355-362).  ids, weights [Q][cap]: the first min(n[q], cap) entries, the rest untouched; n[q]: the full length; counters [Q][K]
 * (may be NULL): mConnectedKeyFrameWeights with 0 for an absent key. */
typedef struct { int32_t th, cap; int32_t *ids, *weights, *n, *counters; } orbc_connections_t;
/* KeyFrameCulling over the queries in the order of vpLocalKeyFrames: the result of the reference's SEQUENTIAL loop, in which
 * pKF->SetBadFlag() changes what later keyframes see (src/KeyFrame.cc:454-472, src/MapPoint.cc:121-178).  With C the set of query
 * keyframes culled so far: an observation by a keyframe in C is gone; a point's nObs is the sum over its remaining observations of
 * stereo ? 2 : 1; a point is bad if it was bad on entry, or lost at least one observation and has nObs <= 2 left.  Per query: id == 0:
 * verdict 0, counts 0.  A feature is skipped if its point is -1 or bad, or if !monocular && (depth > th_depth || depth < 0); otherwise
 * n_mps++, and n_redundant++ if nObs > th_obs (the reference: 3) and at least th_obs remaining observations by other keyframes have
 * octave_i <= octave + 1.  verdict = (double)n_redundant > 0.9 * (double)n_mps ? (not_erase ? 2 : 1) : 0; 1 joins C, 2 is
 * mbToBeErased and does not.  point_bad [P] (may be NULL): every point's flag after the whole loop. */
typedef struct { int32_t monocular, th_obs; int32_t *n_mps, *n_redundant, *verdict; uint8_t *point_bad; } orbc_culling_t;
/* Any of the three results of one table in ONE upload: a NULL conn / cull / normals is not computed (the queries of a NULL result may
 * be NULL too).  All three see the table as it is on entry.  normals [P]: what host/frame_shim.h's MapPoint::UpdateNormalAndDepth
 * pins: normali = pos - Ow_i in float, its squared norm a double sum in the order 0 1 2, inv = (float)(1.0 / sqrt(s)),
 * normal = normali * inv + normal as a separate multiply and add, the observations strictly in list order, dist = (float)norm(pos -
 * Ow_ref), max = dist * sf[octave of the reference keyframe's observation], min = max / sf[nlevels - 1] correctly rounded,
 * normal_out = (float)((double)normal * (1.0 / n)). */
int orbc_covisibility(const orbc_table_t *table, const orbc_queries_t *conn_queries, const orbc_connections_t *conn,
                      const orbc_queries_t *cull_queries, const orbc_culling_t *cull, orbc_normal_t *normals, int device);
int orbc_update_connections(const orbc_table_t *table, const orbc_queries_t *queries, int th, int cap, int32_t *ids, int32_t *weights,
                            int32_t *n, int32_t *counters, int device);
int orbc_keyframe_culling(const orbc_table_t *table, const orbc_queries_t *queries, int monocular, int th_obs, int32_t *n_mps,
                          int32_t *n_redundant, int32_t *verdict, uint8_t *point_bad, int device);
int orbc_update_normal_and_depth(const orbc_table_t *table, orbc_normal_t *normals, int device);

/* ------------------------------------------------------------------------------------------------------------------------------
 * The local map: Tracking::UpdateLocalMap (src/Tracking.cc:1340-1484: UpdateLocalKeyFrames + UpdateLocalPoints) on a snapshot of the
 * map that stays on the device (row a34, prefix orbt_).  DESIGN.md section 6, "k_lm_*".
 *
 * A handle holds one snapshot and the per-frame state; orbt_localmap_set_map replaces the snapshot with one upload when the map
 * changed, orbt_update_local_map is the one call per tracked frame: N point indices up, the local lists down.  One handle is used by
 * one thread at a time.  The handle's buffers only grow.  orbt_localmap_create touches no device.
 *
 * The snapshot: `table` is the observation table of the orbc_ section, unchanged (slot order stands for the reference's pointer
 * order); `features` are every keyframe's GetMapPointMatches(): Q == K and query_kf[q] == q, and only feat[].point is read;
 * parent[K]: slot of GetParent() or -1; cov_off[K + 1] / cov[]: GetVectorCovisibleKeyFrames() as slots, in the ordered list's order;
 * child_off[K + 1] / child[]: GetChilds() as slots, ascending (the reference walks a std::set<KeyFrame*>: a stated difference of the
 * same kind as the table's); views[P]; desc[P][32]: GetDescriptor().
 * Every index range and offset array is checked on the host in the packing pass: ORBX_ERR_ARG with a message before a device is
 * touched.  K > ORBC_MAX_CULL_KEYFRAMES (the marks are one bit per slot in LDS): ORBX_ERR_UNSUPPORTED.  No usable GPU:
 * ORBX_ERR_NO_DEVICE; the handle then has no snapshot, and orbt_update_local_map still checks its arguments against that map's K and
 * P (ORBX_ERR_ARG) before it returns ORBX_ERR_NO_DEVICE. */
typedef struct { float normal[3];       /* GetNormal() */
                 float max_distance;    /* mfMaxDistance */
                 float min_distance;    /* mfMinDistance */
                 int32_t observations;  /* Observations(): nObs */
} orbt_pointview_t;                     /* 24 B */
typedef struct { const orbc_table_t *table; const orbc_queries_t *features; const int32_t *parent; const int32_t *cov_off, *cov;
                 const int32_t *child_off, *child; const orbt_pointview_t *views; const uint8_t *desc; } orbt_map_t;
#define ORBT_END_RAN_OUT 0              /* every first-stage keyframe was visited */
#define ORBT_END_LENGTH 1               /* the list was longer than max_keyframes (src/Tracking.cc:1430) */
#define ORBT_END_PARENT 2               /* a parent was appended: the `break` at :1473 leaves the loop over the keyframes */
typedef struct { int32_t empty_vote, n_voted, ref_kf, ref_votes, extension_end, launches, syncs, pad; } orbt_local_info_t;   /* 32 B */
/* The result of one frame; the caller owns the arrays: frame_points, holder, ext_obs [N]; local_kf [K]; local_pts, pts [P];
 * mp_desc [P][32].  Only the used prefix of local_kf / local_pts / pts / mp_desc is written. */
typedef struct { int32_t *frame_points, *holder, *ext_obs; int32_t *local_kf; int32_t *local_pts; orbm_worldpoint_t *pts; uint8_t *mp_desc;
                 int32_t n_local_kf, n_local_pts; orbt_local_info_t info; } orbt_local_t;
typedef struct orbt_localmap orbt_localmap_t;
int orbt_localmap_create(int device, orbt_localmap_t **out);
void orbt_localmap_destroy(orbt_localmap_t *h);
/* K, P, the total feature count and the snapshot's bytes of the last orbt_localmap_set_map whose checks passed; device_bytes: what
 * the handle holds on the device.  Any pointer may be NULL */
int orbt_localmap_info(const orbt_localmap_t *h, int *K, int *P, int64_t *features, size_t *snapshot_bytes, size_t *device_bytes);
int orbt_localmap_set_map(orbt_localmap_t *h, const orbt_map_t *map);
/* One frame.  frame_points[i]: the point index of mCurrentFrame.mvpMapPoints[i] or -1; prev_kf[n_prev]: the previous local
 * keyframes, distinct slots.  The result is that of the reference's sequential code:
 * 0. fp[i] = -1 if the point is bad, else frame_points[i] (:1382-1394, :1296-1299) -> out->frame_points.
 * 1. counter[k] = the number of (feature i, observation o) pairs with fp[i] >= 0 and o in that point's list with o.kf == k; a point
 *    named by two features counts twice; a bad keyframe's counter counts like any other (:1380-1396).
 * 2. Every counter 0: info.empty_vote = 1, the local keyframes are prev_kf unchanged, n_voted = 0, ref_kf = -1 (the caller keeps
 *    its reference keyframe); continue at 5 (:1398-1399).
 * 3. The slots with counter > 0 and !bad in ascending slot order; n_voted = their number S; ref_kf = the largest counter's, among
 *    equals the smallest slot, -1 if S == 0 (the list is then empty, not the previous one: :1404 cleared it); ref_votes its counter.
 * 4. For j = 0 .. S-1 over the first-stage entries only (appended keyframes are never visited; where the reference's
 *    reserve(3 * size) would be exceeded its iterators are undefined: the index walk is the stated reading): if the list is longer
 *    than max_keyframes (the reference: 80) stop - a list of exactly 80 still runs, so it can end at 83.  With kf the j-th entry, in
 *    order, each step seeing the marks of the ones before: (a) of the first min(nbest, len) entries (the reference: 10) of kf's
 *    covisible list the first that is not bad and not in the list is appended; (b) of kf's children the first that is not bad and
 *    not in the list is appended; (c) if parent >= 0 and it is not in the list it is appended, its bad flag NOT tested (:1466-1469),
 *    and THE WHOLE LOOP ENDS: the `break` at :1473 stands in no inner loop.
 * 5. UpdateLocalPoints (:1350-1373): the local keyframes in list order, each one's features in slot order; a point index >= 0 that is
 *    not yet listed and not bad is appended.
 * 6. What SearchLocalPointsHIP (host/ORBmatcher.cc) packs for orbm_search_local_points, byte for byte: pts[j].observations always;
 *    valid = 1 and the nine floats only if the point is named by no fp[i] (mnLastFrameSeen, :1303, :1315), otherwise the record is 0
 *    but for observations; mp_desc[j] the descriptor, or 32 zero bytes where valid == 0; holder[i] = -1 where fp[i] < 0, the local
 *    index of fp[i] where it is listed, else -2 with ext_obs[i] = that point's observations; ext_obs[i] = 0 elsewhere.
 * At most two stream synchronisations per call (info.syncs): the lengths, then the used prefixes. */
int orbt_update_local_map(orbt_localmap_t *h, const int32_t *frame_points, int N, const int32_t *prev_kf, int n_prev, int max_keyframes,
                          int nbest, orbt_local_t *out);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Loop map correction: the two map-sized loops of LoopClosing (row a36, prefix orbr_).  DESIGN.md section 6, "k_mc_*".
 * orbr_correct_loop is src/LoopClosing.cc:444-525 without the UpdateConnections() of :524, which reads no position (the caller runs
 * orbc_update_connections on the same table); orbr_spread_global_ba is :685-746, what follows Optimizer::GlobalBundleAdjustemnt.
 * Every index range is checked on the host in the packing pass: ORBX_ERR_ARG with a message before a device is touched.  No usable GPU:
 * ORBX_ERR_NO_DEVICE after these checks; there is no CPU path.  Scratch, pinned mirror and stream are per host thread
 * (orbx_thread_release_scratch).
 *
 * orbr_correct_loop.  table: the observation table of the orbc_ section, unchanged.  conn: mvpCurrentConnectedKFs with their
 * GetMapPointMatches(); only feat[].point is read.  query_kf is STRICTLY ASCENDING: slot order stands for the pointer order of the
 * reference's std::map<KeyFrame*, g2o::Sim3> CorrectedSim3 (the stated difference of the orbc_ section).  cur: the slot of mpCurrentKF,
 * one of the queries.  Tiw16 [Q][16]: GetPose() of each query.  Scw: mg2oScw.
 * Per query: Twc of cur as KeyFrame::SetPose derives it from Tiw16[cur] (Ow = -Rwc * tcw), Tic = Tiw * Twc (a float 4x4 product, each
 * entry a double sum left to right narrowed once), corrected = Sim3(Ric, tic, 1.0) * Scw (Scw itself for cur), non_corrected =
 * Sim3(Riw, tiw, 1.0), Tiw_new = [R(corrected.q), corrected.t * (1. / s); 0 0 0 1] narrowed, Ow_new = SetPose's centre of Tiw_new.
 * Per point: a point that is not bad and that a query's feature names belongs to the query of the SMALLEST position that names it
 * (what mnCorrectedByKF == mpCurrentKF->mnId leaves behind; a point named twice by one keyframe is corrected once).  There is no
 * mnCorrectedByKF input: a point can only carry the current keyframe's id on entry if that id is 0, and keyframe 0 cannot close a loop.
 * pos' = (float) corrected[owner]^-1.map(non_corrected[owner].map((double) pos)); then UpdateNormalAndDepth on pos' with the arithmetic
 * of orbc_covisibility, in which an observer's (and the reference keyframe's) camera centre is Ow_new if that keyframe is a query at a
 * position strictly below the owner's and the table's Ow otherwise: the owner's own SetPose comes after its point loop (:522).
 * Outputs (all required): corrected, non_corrected [Q]; Tiw_new16 [Q][16]; Ow_new3 [Q][3]; pos3 [P][3] (the input where no query
 * owns the point); corrected_ref [P]: the owner's slot (mnCorrectedReference), -1 for an untouched point; normals [P]: the ORBC_NORMAL_*
 * codes apply to an owned point (a point with an empty list is still moved and reports ORBC_NORMAL_NO_OBSERVATION), and
 * ORBR_NORMAL_UNTOUCHED marks a point that no query owns, the five floats 0.
 * ORBX_ERR_ARG: what the orbc_ section checks of a table and a query set, query_kf not strictly ascending, cur not among the queries,
 * a NULL pointer.  One call is one upload, three launches, one download and one stream synchronisation. */
#define ORBR_NORMAL_UNTOUCHED 4
typedef struct { orbg_sim3_t *corrected, *non_corrected; float *Tiw_new16, *Ow_new3, *pos3; int32_t *corrected_ref; orbc_normal_t *normals; } orbr_loop_out_t;
int orbr_correct_loop(const orbc_table_t *table, const orbc_queries_t *conn, int32_t cur, const float *Tiw16, const orbg_sim3_t *Scw,
                      const orbr_loop_out_t *out, int device);
/* orbr_spread_global_ba.  Tcw16 [K][16]: GetPose(); TcwGBA16 [K][16]: mTcwGBA (read only where kf_in_gba); kf_in_gba [K]:
 * mnBAGlobalForKF == nLoopKF; child_off [K + 1] / child: GetChilds() as slots, as in orbt_map_t; origins [n_origins]:
 * mvpKeyFrameOrigins as slots; pos3, posGBA3 [P][3]; pt_in_gba [P]; ref_kf [P]: slot of GetReferenceKeyFrame() or -1; bad [P].
 * The host finds the keyframes the reference's walk reaches from the origins THROUGH THE CHILD LISTS (a bad keyframe keeps its parent
 * but is in nobody's child set, src/KeyFrame.cc:480-539, and is not reached) and, for each reached keyframe outside the global BA, its
 * level: the distance to the nearest reached ancestor inside it.  One launch per level: TcwGBA_child = (Tcw_child * Twc_parent) *
 * TcwGBA_parent, two float 4x4 products in that order, Twc_parent from the parent's pose on entry as SetPose left it.  A keyframe is
 * marked if it is in the global BA or reached.  Then per point: bad: untouched; pt_in_gba: posGBA; reference keyframe marked and
 * reached: Xc = Rcw_bef * pos + tcw_bef with the pose on entry, pos = Rwc * Xc + twc with the Twc SetPose derives from the new pose;
 * otherwise untouched.
 * Outputs (all required): Tcw_new16 [K][16]: TcwGBA_out of a reached keyframe, the input pose otherwise; TcwGBA_out16 [K][16];
 * kf_marked [K]; kf_reached [K] (may be NULL): the keyframes the walk popped, whose mTcwBefGBA and SetPose the caller owes (:706-707);
 * pos_out3 [P][3]; status [P]: ORBR_SPREAD_*; levels: written by the call, the number of launches over the tree.
 * ORBX_ERR_ARG: an index out of range, offsets that do not start at 0 or decrease, a keyframe in two child lists or in its own, an
 * origin that is in a child list, is repeated, or is outside the global BA (the reference would SetPose an empty matrix), a NULL
 * pointer.  One call is one upload, one launch per level and one for the points, one download and one stream synchronisation. */
#define ORBR_SPREAD_UNTOUCHED 0
#define ORBR_SPREAD_GBA 1                /* took mPosGBA (:724) */
#define ORBR_SPREAD_MOVED 2              /* moved with its reference keyframe (:735-744) */
#define ORBR_SPREAD_UNDEFINED 3          /* ref_kf is -1, or a marked keyframe the walk did not reach (its mTcwBefGBA is empty): the reference is undefined there; untouched */
typedef struct { int32_t K; const float *Tcw16, *TcwGBA16; const uint8_t *kf_in_gba; const int32_t *child_off, *child; const int32_t *origins;
                 int32_t n_origins, P; const float *pos3, *posGBA3; const uint8_t *pt_in_gba; const int32_t *ref_kf; const uint8_t *bad; } orbr_spread_in_t;
typedef struct { float *Tcw_new16, *TcwGBA_out16; uint8_t *kf_marked, *kf_reached; float *pos_out3; int32_t *status; int32_t levels; } orbr_spread_out_t;
int orbr_spread_global_ba(const orbr_spread_in_t *in, orbr_spread_out_t *out, int device);

/* The host-array matcher entry points keep grow-only device scratch, a pinned mirror and one non-blocking stream
 * PER HOST THREAD (re-entrant without locks: the reference calls matchers from Tracking, LocalMapping and LoopClosing
 * threads at once, src/LocalMapping.cc:223, src/LoopClosing.cc:249).  Nothing is freed implicitly; a thread calls
 * this before it exits or to hand the memory back.  Safe to call at any time, any number of times. */
int orbx_thread_release_scratch(void);

const char *orbx_last_error(void);      /* thread-local description of the last failure */
const char *orbx_version(void);
int orbx_device_count(void);            /* number of HIP devices visible (0 if none) */

#ifdef __cplusplus
}
#endif
#endif /* ORBX_H */
