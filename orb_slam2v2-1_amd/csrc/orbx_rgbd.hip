// orbx_rgbd.hip — MI355X (gfx950) RGB-D front end: hand-written HIP kernels + C ABI.
//
//   k_gray_from_color   Tracking::GrabImageRGBD's cvtColor(RGB/BGR[A]2GRAY)      (src/Tracking.cc:315-333)
//   k_rgbd_assoc        Frame::UndistortKeyPoints + Frame::ComputeStereoFromRGBD  (src/Frame.cc:419-449, 658-679),
//                       with GrabImageRGBD's depth convertTo applied to the sampled pixel (src/Tracking.cc:335-336)
//   orbx_rgbd_frame     the RGB-D Frame constructor's feature part for one frame, host to host (src/Frame.cc:119-171)
//
// The arithmetic restated here is that of OpenCV 3.2: RGB2Gray<uchar> in 14-bit fixed point, convertTo to CV_32F
// as one float multiply, cvUndistortPoints as five fixed iterations in double.  tests/rgbd_ref.py holds the same restatement in
// numpy, operation by operation.
#include "orbx_internal.h"
#include <math.h>
#include <algorithm>

// RGB2Gray<uchar> (OpenCV 2.4 / 3.x, yuv_shift 14): Y = (R*4899 + G*9617 + B*1868 + 8192) >> 14.  c0 c1 c2 in memory order;
// rgb = 1: c0 is R, else c0 is B.
__device__ __forceinline__ uint32_t gray_px(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t w0, uint32_t w2) {
    return (c0 * w0 + c1 * 9617u + c2 * w2 + 8192u) >> 14;
}

// One thread per 4 output pixels of a row; a block covers 256 pixels x 4 rows of one image.  Streaming: where the four pixels
// lie inside the row and their source is 4-byte (3 channels: one 12-byte load) / 16-byte (4 channels) aligned, the thread reads
// them with one wide load and writes one dword; the row's tail and unaligned rows take byte loads.
#define GC_PX 4
#define GC_TX 64
#define GC_TY 4
template <int CH>
__global__ __launch_bounds__(GC_TX *GC_TY) void k_gray_from_color(const uint8_t *__restrict__ src, size_t srcImg, int srcStride,
                                                                   uint8_t *__restrict__ dst, size_t dstImg, int dstStride, int w,
                                                                   int h, int rgb) {
    const int x0 = (blockIdx.x * GC_TX + threadIdx.x) * GC_PX, y = blockIdx.y * GC_TY + threadIdx.y;
    if (x0 >= w || y >= h) return;
    const uint32_t w0 = rgb ? 4899u : 1868u, w2 = rgb ? 1868u : 4899u;
    const uint8_t *s = src + blockIdx.z * srcImg + (size_t)y * srcStride + (size_t)x0 * CH;
    uint8_t *d = dst + blockIdx.z * dstImg + (size_t)y * dstStride + x0;
    const bool full = x0 + GC_PX <= w;
    if (full && ((uintptr_t)s & (CH == 4 ? 15 : 3)) == 0) {
        uint32_t g;
        if (CH == 4) {
            const uint4 v = *(const uint4 *)s;
            const uint32_t q[4] = {v.x, v.y, v.z, v.w};
            g = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) g |= gray_px(q[i] & 255u, (q[i] >> 8) & 255u, (q[i] >> 16) & 255u, w0, w2) << (8 * i);
        } else {
            const uint32_t a = ((const uint32_t *)s)[0], b = ((const uint32_t *)s)[1], c = ((const uint32_t *)s)[2];
            // bytes: a = r0 g0 b0 r1 | b = g1 b1 r2 g2 | c = b2 r3 g3 b3
            g = gray_px(a & 255u, (a >> 8) & 255u, (a >> 16) & 255u, w0, w2) |
                gray_px(a >> 24, b & 255u, (b >> 8) & 255u, w0, w2) << 8 |
                gray_px((b >> 16) & 255u, b >> 24, c & 255u, w0, w2) << 16 |
                gray_px((c >> 8) & 255u, (c >> 16) & 255u, c >> 24, w0, w2) << 24;
        }
        if (((uintptr_t)d & 3) == 0) {
            *(uint32_t *)d = g;
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) d[i] = (uint8_t)(g >> (8 * i));
        }
        return;
    }
    const int n = min(GC_PX, w - x0);
    for (int i = 0; i < n; i++) d[i] = (uint8_t)gray_px(s[i * CH], s[i * CH + 1], s[i * CH + 2], w0, w2);
}

// The camera as cvUndistortPoints holds it: K and the distortion in double (cvConvert of the CV_32F matrices), k[0..4] =
// k1 k2 p1 p2 k3; the coefficients OpenCV 3.2 also reads (k4..k6, s1..s4) are 0 for a 4- or 5-element mDistCoef.
struct RgbdCam {
    double fx, fy, cx, cy, ifx, ify;
    double k[5];
    float mbf;
    int undistort;   // mDistCoef.at<float>(0) != 0.0 (src/Frame.cc:421)
};

// cvUndistortPoints (OpenCV 3.2, modules/imgproc/src/undistort.cpp) for one point with R = I, P = K, every term written out,
// the ones that are exactly zero here included (tilt = identity, k4..k6 = 0, thin prism s1..s4 = 0, RR = P*R = K), in the order
// OpenCV evaluates them.  Later releases leave the loop early when icdist < 0 - only reachable with distortion far outside real
// lenses, not modelled.
__device__ __forceinline__ void undistort_point(const RgbdCam &c, float u, float v, float &ou, float &ov) {
    const double k4 = 0.0, k5 = 0.0, k6 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
    double x = (double)u, y = (double)v;
    x = (x - c.cx) * c.ifx;
    y = (y - c.cy) * c.ify;
    // invMatTilt * (x, y, 1) with invMatTilt = I, invProj = 1 / vecUntilt(2)
    const double ux = 1.0 * x + 0.0 * y + 0.0 * 1.0, uy = 0.0 * x + 1.0 * y + 0.0 * 1.0, uz = 0.0 * x + 0.0 * y + 1.0 * 1.0;
    const double invProj = uz != 0.0 ? 1. / uz : 1.0;
    const double x0 = invProj * ux, y0 = invProj * uy;
    x = x0; y = y0;
    for (int j = 0; j < 5; j++) {
        const double r2 = x * x + y * y;
        const double icdist = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((c.k[4] * r2 + c.k[1]) * r2 + c.k[0]) * r2);
        const double deltaX = 2 * c.k[2] * x * y + c.k[3] * (r2 + 2 * x * x) + s1 * r2 + s2 * r2 * r2;
        const double deltaY = c.k[2] * (r2 + 2 * y * y) + 2 * c.k[3] * x * y + s3 * r2 + s4 * r2 * r2;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    const double xx = c.fx * x + 0.0 * y + c.cx;
    const double yy = 0.0 * x + c.fy * y + c.cy;
    const double ww = 1. / (0.0 * x + 0.0 * y + 1.0);
    ou = (float)(xx * ww);
    ov = (float)(yy * ww);
}

// One lane per keypoint of B frames: mvKeysUn, then mvuRight / mvDepth from the depth sample at the DISTORTED keypoint
// (imDepth.at<float>(v, u) with u, v truncated).  depth == NULL: the monocular constructor's tail (-1 / -1, :174-228).
// A sample outside the depth image (the reference would read out of bounds) counts as no depth.
__global__ __launch_bounds__(256) void k_rgbd_assoc(const orbx_keypoint_t *__restrict__ kps, const int32_t *__restrict__ counts, int cap,
                                                    const uint8_t *__restrict__ depth, int depthType, int w, int h, int depthStride,
                                                    size_t depthImg, float factor, int convert, RgbdCam cam,
                                                    orbx_keypoint_t *__restrict__ kun, float *__restrict__ uright,
                                                    float *__restrict__ depthOut) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int n = min(counts[b], cap);
    if (i >= n) return;
    const size_t r = (size_t)b * cap + i;
    orbx_keypoint_t kp = kps[r];
    const float u = kp.x, v = kp.y;
    if (cam.undistort) undistort_point(cam, u, v, kp.x, kp.y);
    kun[r] = kp;
    float ur = -1.0f, dp = -1.0f;
    if (depth) {
        const int iu = (int)u, iv = (int)v;
        if (iu >= 0 && iu < w && iv >= 0 && iv < h) {
            const uint8_t *row = depth + b * depthImg + (size_t)iv * depthStride;
            float d;
            if (depthType == ORBX_DEPTH_U16) d = (float)((const uint16_t *)row)[iu] * factor;   // convertTo(CV_32F, factor): always
            else {
                d = ((const float *)row)[iu];
                if (convert) d = d * factor;
            }
            if (d > 0) {
                dp = d;
                ur = kp.x - cam.mbf / d;
            }
        }
    }
    uright[r] = ur;
    depthOut[r] = dp;
}

static int no_device() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
        (void)hipGetLastError();
        orbx_set_error("no usable HIP device");
        return ORBX_ERR_NO_DEVICE;
    }
    return ORBX_OK;
}

static int launch_gray(const uint8_t *d_color, int B, int w, int hgt, int channels, int rgb, int stride, size_t image_stride,
                       uint8_t *d_gray, int gray_stride, size_t gray_image_stride, hipStream_t st) {
    const dim3 grid((w + GC_TX * GC_PX - 1) / (GC_TX * GC_PX), (hgt + GC_TY - 1) / GC_TY, B), block(GC_TX, GC_TY);
    (void)hipGetLastError();
    if (channels == 3)
        hipLaunchKernelGGL(k_gray_from_color<3>, grid, block, 0, st, d_color, image_stride, stride, d_gray, gray_image_stride, gray_stride,
                           w, hgt, rgb ? 1 : 0);
    else
        hipLaunchKernelGGL(k_gray_from_color<4>, grid, block, 0, st, d_color, image_stride, stride, d_gray, gray_image_stride, gray_stride,
                           w, hgt, rgb ? 1 : 0);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbx_gray_from_color_device(const uint8_t *d_color, int B, int w, int hgt, int channels, int rgb, int stride,
                                           size_t image_stride_bytes, uint8_t *d_gray, int gray_stride,
                                           size_t gray_image_stride_bytes, void *stream) {
    if (!d_color || !d_gray || B < 1 || B > 65535 || w < 1 || hgt < 1 || (channels != 3 && channels != 4) ||
        (size_t)stride < (size_t)w * channels || gray_stride < w ||
        (B > 1 && (image_stride_bytes < (size_t)stride * hgt || gray_image_stride_bytes < (size_t)gray_stride * hgt))) {
        orbx_set_error("orbx_gray_from_color_device: bad arguments");
        return ORBX_ERR_ARG;
    }
    int rc = no_device();
    if (rc) return rc;
    return launch_gray(d_color, B, w, hgt, channels, rgb, stride, image_stride_bytes, d_gray, gray_stride, gray_image_stride_bytes,
                       (hipStream_t)stream);
}

static bool bad_camera(const orbx_rgbd_camera_t *c) {
    return !c || !(c->fx != 0.0f) || !(c->fy != 0.0f);
}

static RgbdCam rgbd_cam(const orbx_rgbd_camera_t *c) {
    RgbdCam r;
    r.fx = c->fx; r.fy = c->fy; r.cx = c->cx; r.cy = c->cy;
    r.ifx = 1. / r.fx; r.ify = 1. / r.fy;
    r.k[0] = c->k1; r.k[1] = c->k2; r.k[2] = c->p1; r.k[3] = c->p2; r.k[4] = c->k3;
    r.mbf = c->mbf;
    r.undistort = c->k1 == 0.0f ? 0 : 1;   // if(mDistCoef.at<float>(0)==0.0) mvKeysUn = mvKeys (src/Frame.cc:421-425)
    return r;
}

// GrabImageRGBD (src/Tracking.cc:335-336): convertTo(CV_32F, mDepthMapFactor) unless the image is CV_32F already and the factor is 1
static int depth_converts(int depth_type, float factor) {
    return (fabs(factor - 1.0f) > 1e-5 || depth_type != ORBX_DEPTH_F32) ? 1 : 0;
}

static int launch_assoc(const orbx_keypoint_t *d_kps, const int32_t *d_counts, int B, int cap, const void *d_depth, int depth_type,
                        int w, int hgt, int depth_stride, size_t depth_image_stride, float factor, const orbx_rgbd_camera_t *cam,
                        orbx_keypoint_t *d_kun, float *d_uright, float *d_depth_out, hipStream_t st) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_rgbd_assoc, dim3((cap + 255) / 256, B), dim3(256), 0, st, d_kps, d_counts, cap, (const uint8_t *)d_depth,
                       depth_type, w, hgt, depth_stride, depth_image_stride, factor, depth_converts(depth_type, factor), rgbd_cam(cam),
                       d_kun, d_uright, d_depth_out);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

static size_t depth_esize(int t) { return t == ORBX_DEPTH_U16 ? 2 : 4; }

extern "C" int orbm_rgbd_batch_device(const orbx_keypoint_t *d_kps, const int32_t *d_counts, int B, int cap, const void *d_depth,
                                      int depth_type, int w, int hgt, int depth_stride, size_t depth_image_stride_bytes,
                                      float depth_map_factor, const orbx_rgbd_camera_t *cam, orbx_keypoint_t *d_kun, float *d_uright,
                                      float *d_depth_out, void *stream) {
    if (!d_kps || !d_counts || !d_kun || !d_uright || !d_depth_out || B < 1 || B > 65535 || cap < 1 || bad_camera(cam) ||
        (d_depth && ((depth_type != ORBX_DEPTH_U16 && depth_type != ORBX_DEPTH_F32) || w < 1 || hgt < 1 ||
                     (size_t)depth_stride < (size_t)w * depth_esize(depth_type) || (depth_stride & (depth_esize(depth_type) - 1)) ||
                     (B > 1 && depth_image_stride_bytes < (size_t)depth_stride * hgt)))) {
        orbx_set_error("orbm_rgbd_batch_device: bad arguments");
        return ORBX_ERR_ARG;
    }
    int rc = no_device();
    if (rc) return rc;
    return launch_assoc(d_kps, d_counts, B, cap, d_depth, depth_type, w, hgt, depth_stride, depth_image_stride_bytes, depth_map_factor,
                        cam, d_kun, d_uright, d_depth_out, (hipStream_t)stream);
}

// ---- orbx_rgbd_frame: handle-owned scratch
// device block [kps | desc | kun | uright | depth | counts] of `cap` rows (one copy down), its pinned mirror, the colour / gray /
// depth images, and the event that orders the association behind the depth upload on the handle's second side stream
struct RgbdScratch {
    uint8_t *d_out, *h_out; int cap;
    uint8_t *d_color; size_t colorBytes;
    uint8_t *d_gray; size_t grayBytes;
    uint8_t *d_depth; size_t depthBytes;
    hipEvent_t evDepth;
};
struct RgbdOut {
    size_t kps, desc, kun, ur, dp, cnt, bytes;
};
static RgbdOut rgbd_layout(int cap) {
    RgbdOut o;
    o.kps = 0;
    o.desc = o.kps + sizeof(orbx_keypoint_t) * (size_t)cap;
    o.kun = o.desc + 32 * (size_t)cap;
    o.ur = o.kun + sizeof(orbx_keypoint_t) * (size_t)cap;
    o.dp = o.ur + 4 * (size_t)cap;
    o.cnt = o.dp + 4 * (size_t)cap;
    o.bytes = o.cnt + 16;
    return o;
}

void orbx_internal_free_rgbd_scratch(orbx_extractor *h) {
    RgbdScratch *s = h->rgbd;
    if (!s) return;
    hipFree(s->d_out); if (s->h_out) hipHostFree(s->h_out);
    hipFree(s->d_color); hipFree(s->d_gray); hipFree(s->d_depth);
    if (s->evDepth) hipEventDestroy(s->evDepth);
    delete s;
    h->rgbd = nullptr;
}

static int grow(uint8_t **p, size_t *have, size_t need) {
    need = ((need + 255) & ~(size_t)255) + 256;   // (as the host API's staging: whole 256-byte blocks and one more)
    if (*have >= need) return ORBX_OK;
    hipFree(*p); *p = nullptr; *have = 0;
    ORBX_HIP(scratch_malloc(p, need));
    *have = need;
    return ORBX_OK;
}

extern "C" int orbx_rgbd_frame(orbx_extractor_t *h, const uint8_t *img, int channels, int rgb, int w, int hgt, int stride,
                               const void *depth, int depth_type, int depth_stride, float depth_map_factor,
                               const orbx_rgbd_camera_t *cam, int cap, orbx_keypoint_t *kp, uint8_t *desc, int *n,
                               orbx_keypoint_t *kun, float *uright, float *depth_out) {
    if (!h || !kp || !desc || !n || !kun || !uright || !depth_out || cap < 1 || (channels != 1 && channels != 3 && channels != 4) ||
        bad_camera(cam) || (depth && depth_type != ORBX_DEPTH_U16 && depth_type != ORBX_DEPTH_F32)) {
        orbx_set_error("orbx_rgbd_frame: bad arguments");
        return ORBX_ERR_ARG;
    }
    *n = 0;
    if (!img || w <= 0 || hgt <= 0) return ORBX_OK;   // empty image (src/ORBextractor.cc:1046-1047)
    if ((size_t)stride < (size_t)w * channels) { orbx_set_error("orbx_rgbd_frame: stride < width * channels"); return ORBX_ERR_ARG; }
    if (depth && ((size_t)depth_stride < (size_t)w * depth_esize(depth_type) || (depth_stride & (depth_esize(depth_type) - 1)))) {
        orbx_set_error("orbx_rgbd_frame: bad depth stride %d", depth_stride);
        return ORBX_ERR_ARG;
    }
    ORBX_HIP(hipSetDevice(h->device));
    if (!h->rgbd) h->rgbd = new RgbdScratch();   // (zero-initialised)
    RgbdScratch *s = h->rgbd;
    if (!s->evDepth) ORBX_HIP(hipEventCreateWithFlags(&s->evDepth, hipEventDisableTiming));
    // rows: enough for any frame (every level returns at most max(N + 2, 4 * nIni) nodes, nIni <= ORBX_MAX_ROOTS), so that the count
    // the caller's cap is checked against is never clamped itself
    const int dcap = std::max(cap, std::max(orbx_max_keypoints(h), h->nfeatures + h->nlevels * (3 + 4 * ORBX_MAX_ROOTS)));
    const RgbdOut L = rgbd_layout(dcap);
    if (s->cap < dcap) {
        hipFree(s->d_out); s->d_out = nullptr;
        if (s->h_out) { hipHostFree(s->h_out); s->h_out = nullptr; }
        s->cap = 0;
        ORBX_HIP(scratch_malloc(&s->d_out, L.bytes));
        ORBX_HIP(scratch_host_malloc((void **)&s->h_out, L.bytes, hipHostMallocDefault));
        s->cap = dcap;
    }
    hipStream_t st = h->stream;
    const uint8_t *d_gray;
    int gstride;
    const size_t span = (size_t)stride * (hgt - 1) + (size_t)w * channels;
    if (channels == 1) {   // gray already: extracted from where it lands
        int rc = grow(&s->d_gray, &s->grayBytes, span);
        if (rc) return rc;
        ORBX_HIP(hipMemcpyAsync(s->d_gray, img, span, hipMemcpyHostToDevice, st));
        d_gray = s->d_gray; gstride = stride;
    } else {
        gstride = (w + 63) & ~63;
        int rc = grow(&s->d_color, &s->colorBytes, span);
        if (!rc) rc = grow(&s->d_gray, &s->grayBytes, (size_t)gstride * hgt);
        if (rc) return rc;
        ORBX_HIP(hipMemcpyAsync(s->d_color, img, span, hipMemcpyHostToDevice, st));
        rc = launch_gray(s->d_color, 1, w, hgt, channels, rgb, stride, span, s->d_gray, gstride, (size_t)gstride * hgt, st);
        if (rc) return rc;
        d_gray = s->d_gray;
    }
    uint8_t *o = s->d_out;
    orbx_keypoint_t *d_kps = (orbx_keypoint_t *)(o + L.kps);
    int32_t *d_cnt = (int32_t *)(o + L.cnt);
    int rc = orbx_extract_batch_device(h, d_gray, 1, w, hgt, gstride, (size_t)gstride * hgt, d_kps, o + L.desc, d_cnt, dcap, st);
    if (rc) return rc;
    const uint8_t *d_dep = nullptr;
    if (depth) {   // the depth image goes up on a side stream while the extraction runs
        const size_t dspan = (size_t)depth_stride * (hgt - 1) + (size_t)w * depth_esize(depth_type);
        rc = grow(&s->d_depth, &s->depthBytes, dspan);
        if (rc) return rc;
        hipStream_t up = h->side[ORBX_SIDE_STREAMS - 1];
        ORBX_HIP(hipMemcpyAsync(s->d_depth, depth, dspan, hipMemcpyHostToDevice, up));
        ORBX_HIP(hipEventRecord(s->evDepth, up));
        ORBX_HIP(hipStreamWaitEvent(st, s->evDepth, 0));
        d_dep = s->d_depth;
    }
    rc = launch_assoc(d_kps, d_cnt, 1, dcap, d_dep, depth_type, w, hgt, depth_stride, 0, depth_map_factor, cam,
                      (orbx_keypoint_t *)(o + L.kun), (float *)(o + L.ur), (float *)(o + L.dp), st);
    if (rc) return rc;
    ORBX_HIP(hipMemcpyAsync(s->h_out, s->d_out, L.bytes, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    const uint8_t *ho = s->h_out;
    int cnt = *(const int32_t *)(ho + L.cnt), status = ORBX_OK;
    if (cnt > cap) {
        orbx_set_error("rgbd frame produced %d keypoints, cap %d", cnt, cap);
        status = ORBX_ERR_CAPACITY;
        cnt = cap;
    }
    *n = cnt;
    if (cnt > 0) {
        memcpy(kp, ho + L.kps, sizeof(orbx_keypoint_t) * cnt);
        memcpy(desc, ho + L.desc, (size_t)32 * cnt);
        memcpy(kun, ho + L.kun, sizeof(orbx_keypoint_t) * cnt);
        memcpy(uright, ho + L.ur, sizeof(float) * cnt);
        memcpy(depth_out, ho + L.dp, sizeof(float) * cnt);
    }
    return status;
}
