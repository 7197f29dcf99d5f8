// orbx_rectify.hip — MI355X (gfx950) stereo rectification of raw images: hand-written HIP kernels + C ABI.
//
//   k_rect_map       cv::initUndistortRectifyMap(K, D, R, P[:, :3], size, CV_32FC1)   (ros_stereo.cc:106-107), once per camera
//   k_remap<CH>      cv::remap(raw, rect, M1, M2, INTER_LINEAR) on 8U               (ros_stereo.cc:161-162), per frame, fused
//                    with GrabImageStereo's cvtColor(RGB[A]/BGR[A]2GRAY) for colour input  (src/Tracking.cc:275-310)
//   orbx_stereo_frame_rectified / _view_rectified: both, then the stereo Frame constructor's feature part
//
// The arithmetic restated here is that of OpenCV 2.4.11 / 3.2: the map in double with the row
// recurrence written out, remap in 5-bit fixed point.  tests/rectify_ref.py holds the same restatement in numpy, operation by
// operation.
#include "orbx_internal.h"
#include "orbx_div_rn.h"
#include <math.h>
#include <algorithm>

// Output tile of k_remap: 64 x 16 pixels, 256 lanes, 4 consecutive pixels of one row per lane.
#define RT_W 64
#define RT_H 16
// A tile reads its source footprint into LDS when the footprint's bounding box has at most this many pixels (16 KiB of 4-channel
// pixels); larger footprints (strong distortion, rotation, maps that leave the image) gather every tap from memory instead.
#define RT_LDS_PX 4096
// images one workgroup of k_remap filters with the map entries it loaded once
#define RT_IPG 8
#define RT_MAX_DIM 4095

struct RectTile {
    int x0, y0, x1, y1;   // bounding box [x0, x1) x [y0, y1) of the taps with non-negative coordinates; empty: x0 >= x1
    int gather, pad[3];
};

struct orbx_rectifier {
    int device, w, h, tilesX, tilesY, ntiles, ngather;
    int ldsBytes[5];      // dynamic LDS of k_remap<CH> for this map (index CH)
    float *d_mapx, *d_mapy;
    uint2 *d_fix;         // per pixel: sx | sy << 16 (int16 each), ax | ay << 5
    RectTile *d_tiles;
    size_t bytes;
};

// what initUndistortRectifyMap reads: iR = (Ar*R)^-1, K's focal lengths and centre, the 14 distortion slots (unused ones 0)
struct MapCoef {
    double ir[9];
    double fx, fy, u0, v0;
    double k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4;
};

// cvRound(m * 32.0f) as remap computes it on x86 (cvtss2si): round half to even; NaN, +-inf and |.| >= 2^31 give INT_MIN
__device__ __forceinline__ int round_q5(float m) {
    const float v = m * 32.0f;
    return (v >= -2147483648.0f && v < 2147483648.0f) ? (int)rintf(v) : INT_MIN;
}

// One lane per map row: the row recurrence of initUndistortRectifyMap is sequential by definition (_x += ir[0] per column).
// Every term of OpenCV's expression is written out, the ones that are exactly zero here included (k4..k6 unless 8 coefficients,
// s1..s4, the identity tilt), and every division goes through orbx_div_rn.  Writes the CV_32F maps, remap's fixed-point form, and per
// output tile the bounding box of the taps with non-negative coordinates (atomics on [tile][minx, miny, maxx, maxy]).
__global__ __launch_bounds__(64) void k_rect_map(MapCoef c, int w, int h, int tilesX, float *__restrict__ mapx,
                                                 float *__restrict__ mapy, uint2 *__restrict__ fix, int *__restrict__ box) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= h) return;
    const double *ir = c.ir;
    double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
    const size_t row = (size_t)i * w;
    int *tb = box + (size_t)(i / RT_H) * tilesX * 4;
    for (int tx = 0; tx < tilesX; tx++) {
        int bx0 = INT_MAX, by0 = INT_MAX, bx1 = INT_MIN, by1 = INT_MIN;
        const int j1 = min(w, (tx + 1) * RT_W);
        for (int j = tx * RT_W; j < j1; j++, _x += ir[0], _y += ir[3], _w += ir[6]) {
            const double ww = orbx_div_rn(1., _w), x = _x * ww, y = _y * ww;
            const double x2 = x * x, y2 = y * y;
            const double r2 = x2 + y2, _2xy = 2 * x * y;
            const double kr = orbx_div_rn(1 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2, 1 + ((c.k6 * r2 + c.k5) * r2 + c.k4) * r2);
            const double xd = (x * kr + c.p1 * _2xy + c.p2 * (r2 + 2 * x2) + c.s1 * r2 + c.s2 * r2 * r2);
            const double yd = (y * kr + c.p1 * (r2 + 2 * y2) + c.p2 * _2xy + c.s3 * r2 + c.s4 * r2 * r2);
            // vecTilt = matTilt * (xd, yd, 1) with matTilt = I (Matx product: s = 0; s += a(i,k) * b(k))
            const double vt0 = ((0.0 + 1.0 * xd) + 0.0 * yd) + 0.0 * 1.0;
            const double vt1 = ((0.0 + 0.0 * xd) + 1.0 * yd) + 0.0 * 1.0;
            const double vt2 = ((0.0 + 0.0 * xd) + 0.0 * yd) + 1.0 * 1.0;
            const double invProj = vt2 != 0.0 ? orbx_div_rn(1., vt2) : 1;
            const double u = c.fx * invProj * vt0 + c.u0;
            const double v = c.fy * invProj * vt1 + c.v0;
            const float mu = (float)u, mv = (float)v;
            mapx[row + j] = mu;
            mapy[row + j] = mv;
            // remap's conversion of a float map (INTER_LINEAR): X = cvRound(m*32), (sat_i16(X >> 5), X & 31)
            const int X = round_q5(mu), Y = round_q5(mv);
            const int sx = min(max(X >> 5, -32768), 32767), sy = min(max(Y >> 5, -32768), 32767);
            fix[row + j] = make_uint2((uint32_t)(sx & 0xffff) | ((uint32_t)sy << 16), (uint32_t)((X & 31) | ((Y & 31) << 5)));
            if (sx + 1 >= 0 && sy + 1 >= 0) {
                bx0 = min(bx0, max(sx, 0)); by0 = min(by0, max(sy, 0));
                bx1 = max(bx1, sx + 1); by1 = max(by1, sy + 1);
            }
        }
        if (bx0 <= bx1) {
            atomicMin(tb + 4 * tx, bx0); atomicMin(tb + 4 * tx + 1, by0);
            atomicMax(tb + 4 * tx + 2, bx1); atomicMax(tb + 4 * tx + 3, by1);
        }
    }
}

struct RemapArgs {
    const uint2 *fix[2];
    const RectTile *tiles[2];
    const uint8_t *src; size_t srcImg; int srcStride, sw, sh;
    uint8_t *dst; size_t dstImg; int dstStride, w, h, tilesX;
    int B0, B, groups0, rgb;
};

// remap(INTER_LINEAR, BORDER_CONSTANT 0) of one pixel and channel from its four taps, in Q10: the separable form of OpenCV's
// (sum w*p + 16384) >> 15 with the Q15 table w = 32 (32-ay|ay) (32-ax|ax).  Row sums stay below 8161 (16-bit products).
__device__ __forceinline__ uint32_t bilinear(uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11, uint32_t ax, uint32_t ay) {
    const uint32_t t = (32 - ax) * p00 + ax * p01, b = (32 - ax) * p10 + ax * p11;
    return ((32 - ay) * t + ay * b + 512) >> 10;
}

// One workgroup per output tile and group of up to RT_IPG images of one rectifier: the lane's four map entries are loaded once,
// then per image the tile's source footprint (clipped to the image) is read into LDS with aligned dword loads where they lie
// inside a row, the four taps of every pixel are filtered from there, and (3 / 4 channels) the RGB2Gray conversion follows; one
// dword store per lane.  Tiles whose footprint does not fit (marked at map-build time) read every tap from memory instead.  Every
// tap is range-checked against the image (or the clipped box inside it) before its address is formed.
template <int CH>
__global__ __launch_bounds__(256) void k_remap(RemapArgs a) {
    extern __shared__ uint32_t lds[];
    int bx, g;
    xcd_block_map(bx, g);   // neighbouring tiles of an image share source rows: one L2
    const int r = g < a.groups0 ? 0 : 1;
    const int b0 = r == 0 ? g * RT_IPG : a.B0 + (g - a.groups0) * RT_IPG;
    const int b1 = min(b0 + RT_IPG, r == 0 ? a.B0 : a.B);
    const RectTile t = a.tiles[r][bx];
    const int tx = bx % a.tilesX, ty = bx / a.tilesX;
    const int ox = tx * RT_W + (threadIdx.x & 15) * 4, oy = ty * RT_H + (threadIdx.x >> 4);
    const int npx = oy < a.h ? min(max(a.w - ox, 0), 4) : 0;
    int sx[4], sy[4];
    uint32_t ax[4], ay[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint2 f = make_uint2(0x80008000u, 0u);   // (outside every image: reads 0)
        if (k < npx) f = a.fix[r][(size_t)oy * a.w + ox + k];
        sx[k] = (int)(int16_t)(f.x & 0xffff); sy[k] = (int)(int16_t)(f.x >> 16);
        ax[k] = f.y & 31; ay[k] = (f.y >> 5) & 31;
    }
    // the box the taps are read from: the clipped footprint (LDS) or the whole image (gather)
    const bool useLds = !t.gather;
    const int cx0 = useLds ? t.x0 : 0, cy0 = useLds ? t.y0 : 0;
    const int cx1 = useLds ? min(t.x1, a.sw) : a.sw, cy1 = useLds ? min(t.y1, a.sh) : a.sh;
    const int fwB = (cx1 - cx0) * CH, fh = cy1 - cy0;
    const int pitch = (fwB + 6) >> 2;   // dwords per LDS row: the row's bytes plus up to 3 bytes of alignment offset
    const bool any = fwB > 0 && fh > 0;
    const uint32_t w0 = a.rgb ? 4899u : 1868u, w2 = a.rgb ? 1868u : 4899u;
    const uint8_t *ldsB = (const uint8_t *)lds;
    for (int b = b0; b < b1; b++) {
        const uint8_t *S = a.src + (size_t)b * a.srcImg;
        if (useLds) {
            __syncthreads();   // (the previous image's taps are read)
            if (any)
                for (int idx = threadIdx.x; idx < fh * pitch; idx += 256) {
                    const int rr = idx / pitch, k = idx - rr * pitch;
                    const uint8_t *lo = S + (size_t)(cy0 + rr) * a.srcStride + (size_t)cx0 * CH, *hi = lo + fwB;
                    const uint8_t *p = (const uint8_t *)((uintptr_t)lo & ~(uintptr_t)3) + 4 * k;
                    uint32_t v = 0;
                    if (p >= lo && p + 4 <= hi) v = *(const uint32_t *)p;
                    else
                        for (int e = 0; e < 4; e++)
                            if (p + e >= lo && p + e < hi) v |= (uint32_t)p[e] << (8 * e);
                    lds[idx] = v;
                }
            __syncthreads();
        }
        uint32_t out = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t px[CH == 1 ? 1 : 3] = {};
#pragma unroll
            for (int c = 0; c < (CH == 1 ? 1 : 3); c++) {
                uint32_t tap[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int x = sx[k] + (q & 1), y = sy[k] + (q >> 1);
                    uint32_t v = 0;
                    if (x >= cx0 && x < cx1 && y >= cy0 && y < cy1) {
                        if (useLds) {
                            const int rr = y - cy0;
                            const uint32_t off = (uint32_t)(((uintptr_t)S + (size_t)y * a.srcStride + (size_t)cx0 * CH) & 3);
                            v = ldsB[(size_t)rr * pitch * 4 + off + (x - cx0) * CH + c];
                        } else
                            v = S[(size_t)y * a.srcStride + (size_t)x * CH + c];
                    }
                    tap[q] = v;
                }
                px[c] = bilinear(tap[0], tap[1], tap[2], tap[3], ax[k], ay[k]);
            }
            uint32_t o;
            if (CH == 1) o = px[0];
            else o = (px[0] * w0 + px[1] * 9617u + px[2] * w2 + 8192u) >> 14;   // RGB2Gray<uchar> of the remapped pixel
            out |= o << (8 * k);
        }
        if (npx > 0) {
            uint8_t *d = a.dst + (size_t)b * a.dstImg + (size_t)oy * a.dstStride + ox;
            if (npx == 4 && ((uintptr_t)d & 3) == 0) *(uint32_t *)d = out;
            else
                for (int k = 0; k < npx; k++) d[k] = (uint8_t)(out >> (8 * k));
        }
    }
}

// ---- host side
// cv::gemm's 3x3 special case (alpha 1, no C): d(i,j) = a(i,0)*b(0,j) + a(i,1)*b(1,j) + a(i,2)*b(2,j), left to right
static void gemm3(const double *a, const double *b, double *d) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) d[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}
// cv::invert(DECOMP_LU)'s 3x3 special case: det3 by cofactors of row 0, d = 1./d, adjugate * d.  false: singular (d == 0)
static bool invert3(const double *m, double *t) {
#define M(i, j) m[3 * (i) + (j)]
    double d = M(0, 0) * (M(1, 1) * M(2, 2) - M(1, 2) * M(2, 1)) - M(0, 1) * (M(1, 0) * M(2, 2) - M(1, 2) * M(2, 0)) +
               M(0, 2) * (M(1, 0) * M(2, 1) - M(1, 1) * M(2, 0));
    if (d == 0.) return false;
    d = 1. / d;
    t[0] = (M(1, 1) * M(2, 2) - M(1, 2) * M(2, 1)) * d;
    t[1] = (M(0, 2) * M(2, 1) - M(0, 1) * M(2, 2)) * d;
    t[2] = (M(0, 1) * M(1, 2) - M(0, 2) * M(1, 1)) * d;
    t[3] = (M(1, 2) * M(2, 0) - M(1, 0) * M(2, 2)) * d;
    t[4] = (M(0, 0) * M(2, 2) - M(0, 2) * M(2, 0)) * d;
    t[5] = (M(0, 2) * M(1, 0) - M(0, 0) * M(1, 2)) * d;
    t[6] = (M(1, 0) * M(2, 1) - M(1, 1) * M(2, 0)) * d;
    t[7] = (M(0, 1) * M(2, 0) - M(0, 0) * M(2, 1)) * d;
    t[8] = (M(0, 0) * M(1, 1) - M(0, 1) * M(1, 0)) * d;
#undef M
    return true;
}

static void free_rectifier(orbx_rectifier *r) {
    hipFree(r->d_mapx); hipFree(r->d_mapy); hipFree(r->d_fix); hipFree(r->d_tiles);
    delete r;
}

extern "C" int orbx_rectifier_create(const double K[9], const double *D, int nD, const double R[9], const double P3x3[9], int w,
                                     int hgt, int device, orbx_rectifier_t **out) {
    if (out) *out = nullptr;
    if (!out || !K || !R || !P3x3 || !D || (nD != 4 && nD != 5 && nD != 8) || w < 1 || hgt < 1 || w > RT_MAX_DIM ||
        hgt > RT_MAX_DIM) {
        orbx_set_error("orbx_rectifier_create: bad arguments (D: 4, 5 or 8 coefficients; map size 1..%d)", RT_MAX_DIM);
        return ORBX_ERR_ARG;
    }
    MapCoef c;
    memset(&c, 0, sizeof(c));
    double ArR[9];
    gemm3(P3x3, R, ArR);
    if (!invert3(ArR, c.ir)) { orbx_set_error("orbx_rectifier_create: P[:, :3] * R is singular"); return ORBX_ERR_ARG; }
    c.u0 = K[2]; c.v0 = K[5]; c.fx = K[0]; c.fy = K[4];
    c.k1 = D[0]; c.k2 = D[1]; c.p1 = D[2]; c.p2 = D[3];
    c.k3 = nD >= 5 ? D[4] : 0.;
    if (nD >= 8) { c.k4 = D[5]; c.k5 = D[6]; c.k6 = D[7]; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { (void)hipGetLastError(); orbx_set_error("no usable HIP device"); return ORBX_ERR_NO_DEVICE; }
    if (device < 0 || device >= ndev) { orbx_set_error("orbx_rectifier_create: no device %d", device); return ORBX_ERR_ARG; }
    ORBX_HIP(hipSetDevice(device));
    orbx_rectifier *r = new orbx_rectifier();
    r->device = device; r->w = w; r->h = hgt;
    r->tilesX = (w + RT_W - 1) / RT_W; r->tilesY = (hgt + RT_H - 1) / RT_H; r->ntiles = r->tilesX * r->tilesY;
    const size_t npx = (size_t)w * hgt;
    std::vector<int> box((size_t)r->ntiles * 4);
    for (int t = 0; t < r->ntiles; t++) { box[4 * t] = box[4 * t + 1] = INT_MAX; box[4 * t + 2] = box[4 * t + 3] = INT_MIN; }
    int *d_box = nullptr;
    hipStream_t st = nullptr;
    int rc = ORBX_OK;
    auto fail = [&](hipError_t e, const char *what) {
        orbx_set_error("orbx_rectifier_create: %s failed: %s", what, hipGetErrorString(e));
        rc = ORBX_ERR_HIP;
    };
    hipError_t e;
    if ((e = scratch_malloc(&r->d_mapx, npx * 4)) || (e = scratch_malloc(&r->d_mapy, npx * 4)) || (e = scratch_malloc(&r->d_fix, npx * 8)) ||
        (e = scratch_malloc(&r->d_tiles, sizeof(RectTile) * r->ntiles)) || (e = scratch_malloc(&d_box, box.size() * 4)))
        fail(e, "hipMalloc");
    else if ((e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking)))
        fail(e, "hipStreamCreate");
    else if ((e = hipMemcpyAsync(d_box, box.data(), box.size() * 4, hipMemcpyHostToDevice, st)))
        fail(e, "hipMemcpyAsync");
    else {
        (void)hipGetLastError();
        hipLaunchKernelGGL(k_rect_map, dim3((hgt + 63) / 64), dim3(64), 0, st, c, w, hgt, r->tilesX, r->d_mapx, r->d_mapy, r->d_fix, d_box);
        if ((e = hipGetLastError()) || (e = hipMemcpyAsync(box.data(), d_box, box.size() * 4, hipMemcpyDeviceToHost, st)) ||
            (e = hipStreamSynchronize(st)))
            fail(e, "k_rect_map");
    }
    if (rc == ORBX_OK) {
        std::vector<RectTile> tiles(r->ntiles);
        int lds[5] = {0, 0, 0, 0, 0};
        for (int t = 0; t < r->ntiles; t++) {
            RectTile &T = tiles[t];
            memset(&T, 0, sizeof(T));
            const int *bb = &box[4 * t];
            if (bb[0] > bb[2]) continue;   // no tap with non-negative coordinates: reads nothing, writes 0
            T.x0 = bb[0]; T.y0 = bb[1]; T.x1 = bb[2] + 1; T.y1 = bb[3] + 1;
            const long long fw = T.x1 - T.x0, fh = T.y1 - T.y0;
            if (fw * fh > RT_LDS_PX) { T.gather = 1; r->ngather++; continue; }
            for (int ch = 1; ch <= 4; ch++) lds[ch] = std::max(lds[ch], (int)(fh * (((fw * ch + 6) >> 2) * 4)));
        }
        for (int ch = 0; ch < 5; ch++) r->ldsBytes[ch] = std::max(lds[ch], 4);
        if ((e = hipMemcpy(r->d_tiles, tiles.data(), sizeof(RectTile) * r->ntiles, hipMemcpyHostToDevice))) fail(e, "hipMemcpy");
    }
    if (st) hipStreamDestroy(st);
    hipFree(d_box);
    if (rc != ORBX_OK) { free_rectifier(r); return rc; }
    r->bytes = npx * 16 + sizeof(RectTile) * r->ntiles;
    *out = r;
    return ORBX_OK;
}

extern "C" int orbx_rectifier_destroy(orbx_rectifier_t *r) {
    if (!r) return ORBX_OK;
    hipSetDevice(r->device);
    free_rectifier(r);
    return ORBX_OK;
}

extern "C" int orbx_rectifier_maps(const orbx_rectifier_t *r, float *mapx, float *mapy) {
    if (!r) { orbx_set_error("orbx_rectifier_maps: NULL rectifier"); return ORBX_ERR_ARG; }
    ORBX_HIP(hipSetDevice(r->device));
    const size_t n = (size_t)r->w * r->h * 4;
    if (mapx) ORBX_HIP(hipMemcpy(mapx, r->d_mapx, n, hipMemcpyDeviceToHost));
    if (mapy) ORBX_HIP(hipMemcpy(mapy, r->d_mapy, n, hipMemcpyDeviceToHost));
    return ORBX_OK;
}

extern "C" int orbx_rectifier_info(const orbx_rectifier_t *r, int *tiles, int *gather_tiles, size_t *device_bytes) {
    if (!r) { orbx_set_error("orbx_rectifier_info: NULL rectifier"); return ORBX_ERR_ARG; }
    if (tiles) *tiles = r->ntiles;
    if (gather_tiles) *gather_tiles = r->ngather;
    if (device_bytes) *device_bytes = r->bytes;
    return ORBX_OK;
}

static int launch_remap(const orbx_rectifier *r0, const orbx_rectifier *r1, int B0, const uint8_t *d_src, int B, int sw, int sh,
                        int channels, int rgb, int stride, size_t image_stride, uint8_t *d_gray, int gray_stride,
                        size_t gray_image_stride, hipStream_t st) {
    const orbx_rectifier *rr = r0 ? r0 : r1;
    RemapArgs a;
    a.fix[0] = r0 ? r0->d_fix : nullptr; a.fix[1] = r1 ? r1->d_fix : nullptr;
    a.tiles[0] = r0 ? r0->d_tiles : nullptr; a.tiles[1] = r1 ? r1->d_tiles : nullptr;
    a.src = d_src; a.srcImg = image_stride; a.srcStride = stride; a.sw = sw; a.sh = sh;
    a.dst = d_gray; a.dstImg = gray_image_stride; a.dstStride = gray_stride; a.w = rr->w; a.h = rr->h; a.tilesX = rr->tilesX;
    a.B0 = B0; a.B = B; a.groups0 = (B0 + RT_IPG - 1) / RT_IPG; a.rgb = rgb ? 1 : 0;
    const int groups = a.groups0 + (B - B0 + RT_IPG - 1) / RT_IPG;
    int lds = std::max(r0 && B0 > 0 ? r0->ldsBytes[channels] : 4, r1 && B0 < B ? r1->ldsBytes[channels] : 4);
    const dim3 grid(rr->ntiles, groups);
    (void)hipGetLastError();
    if (channels == 1) hipLaunchKernelGGL(k_remap<1>, grid, dim3(256), lds, st, a);
    else if (channels == 3) hipLaunchKernelGGL(k_remap<3>, grid, dim3(256), lds, st, a);
    else hipLaunchKernelGGL(k_remap<4>, grid, dim3(256), lds, st, a);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbx_rectify_device(const orbx_rectifier_t *r0, const orbx_rectifier_t *r1, int B0, const uint8_t *d_src, int B,
                                   int sw, int sh, int channels, int rgb, int stride, size_t image_stride_bytes, uint8_t *d_gray,
                                   int gray_stride, size_t gray_image_stride_bytes, void *stream) {
    const orbx_rectifier *ra = B0 > 0 ? r0 : nullptr, *rb = B0 < B ? r1 : nullptr;
    if (!d_src || !d_gray || B < 1 || B0 < 0 || B0 > B || (B0 > 0 && !r0) || (B0 < B && !r1) || sw < 1 || sh < 1 ||
        (channels != 1 && channels != 3 && channels != 4) || (size_t)stride < (size_t)sw * channels ||
        (ra && rb && (ra->w != rb->w || ra->h != rb->h || ra->device != rb->device))) {
        orbx_set_error("orbx_rectify_device: bad arguments");
        return ORBX_ERR_ARG;
    }
    const orbx_rectifier *rr = ra ? ra : rb;
    const long long groups = (B0 + RT_IPG - 1) / RT_IPG + (B - B0 + RT_IPG - 1) / RT_IPG;
    if (gray_stride < rr->w || groups > 65535 ||
        (B > 1 && (image_stride_bytes < (size_t)stride * sh || gray_image_stride_bytes < (size_t)gray_stride * rr->h))) {
        orbx_set_error("orbx_rectify_device: bad strides or batch");
        return ORBX_ERR_ARG;
    }
    ORBX_HIP(hipSetDevice(rr->device));
    return launch_remap(ra, rb, B0, d_src, B, sw, sh, channels, rgb, stride, image_stride_bytes, d_gray, gray_stride,
                        gray_image_stride_bytes, (hipStream_t)stream);
}

// ---- one stereo frame from a raw pair: handle-owned scratch (raw pair in HBM, its pinned staging, the rectified gray pair)
struct RectScratch {
    uint8_t *d_raw; size_t rawBytes;
    uint8_t *h_stage, *h_stage_dev; size_t stageBytes;
    uint8_t *d_gray; size_t grayBytes;
};

void orbx_internal_free_rect_scratch(orbx_extractor *h) {
    RectScratch *s = h->rect;
    if (!s) return;
    hipFree(s->d_raw); hipFree(s->d_gray);
    if (s->h_stage) hipHostFree(s->h_stage);
    delete s;
    h->rect = nullptr;
}

static int grow_dev(uint8_t **p, size_t *have, size_t need) {
    if (*have >= need) return ORBX_OK;
    hipFree(*p); *p = nullptr; *have = 0;
    ORBX_HIP(scratch_malloc(p, need));
    *have = need;
    return ORBX_OK;
}

static bool bad_rect_args(const orbx_extractor *h, const orbx_rectifier *rl, const orbx_rectifier *rr, int channels, int w,
                          int hgt, int stride, const char *fn) {
    const char *why = nullptr;
    if (!rl || !rr) why = "NULL rectifier";
    else if (channels != 1 && channels != 3 && channels != 4) why = "channels must be 1, 3 or 4";
    else if (w > 0 && hgt > 0 && (rl->w != w || rl->h != hgt || rr->w != w || rr->h != hgt)) why = "rectifier map size differs from the image";
    else if (rl->device != h->device || rr->device != h->device) why = "rectifier on another device";
    else if (w > 0 && hgt > 0 && (size_t)stride < (size_t)w * channels) why = "stride < width * channels";
    if (why) orbx_set_error("%s: %s", fn, why);
    return why != nullptr;
}

// the rectified gray pair of one frame into the handle's scratch, on the handle's stream: image 1 at *d_pair + *gimg
static int rectify_pair(orbx_extractor *h, const orbx_rectifier *rl, const orbx_rectifier *rr, const uint8_t *dl, const uint8_t *dr,
                        int channels, int rgb, int w, int hgt, int stride, const uint8_t **d_pair, int *gstride, size_t *gimg) {
    RectScratch *s = h->rect;
    *gstride = (w + 63) & ~63;
    *gimg = (size_t)*gstride * hgt;
    int rc = grow_dev(&s->d_gray, &s->grayBytes, 2 * *gimg);
    if (rc) return rc;
    hipStream_t st = h->stream;
    // image 1 at dl + (dr - dl): one launch for both (the kernel adds the unsigned, possibly wrapped, difference once)
    const size_t diff = (size_t)((uintptr_t)dr - (uintptr_t)dl);
    rc = launch_remap(rl, rr, 1, dl, 2, w, hgt, channels, rgb, stride, diff, s->d_gray, *gstride, *gimg, st);
    *d_pair = s->d_gray;
    return rc;
}

extern "C" int orbx_stereo_frame_rectified(orbx_extractor_t *h, const orbx_rectifier_t *rl, const orbx_rectifier_t *rr,
                                           const uint8_t *left, const uint8_t *right, int channels, int rgb, int w, int hgt,
                                           int stride, float mbf, float mb, int cap, orbx_keypoint_t *kl, uint8_t *dl, int *nl,
                                           orbx_keypoint_t *kr, uint8_t *dr, int *nr, float *uright, float *depth, int *nmatch) {
    if (!h || !kl || !dl || !nl || !kr || !dr || !nr || !uright || !depth || cap < 1) {
        orbx_set_error("orbx_stereo_frame_rectified: bad arguments");
        return ORBX_ERR_ARG;
    }
    *nl = 0; *nr = 0;
    if (nmatch) *nmatch = 0;
    if (bad_rect_args(h, rl, rr, channels, w, hgt, stride, "orbx_stereo_frame_rectified")) return ORBX_ERR_ARG;
    if (!left || !right || w <= 0 || hgt <= 0) return ORBX_OK;   // empty image (src/ORBextractor.cc:1046-1047)
    ORBX_HIP(hipSetDevice(h->device));
    if (!h->rect) h->rect = new RectScratch();   // (zero-initialised)
    RectScratch *s = h->rect;
    // both raw images go up once (one linear copy each, the caller's row stride kept), then are rectified from HBM
    const size_t span = (size_t)stride * (hgt - 1) + (size_t)w * channels, img = (span + 255) & ~(size_t)255;
    int rc = grow_dev(&s->d_raw, &s->rawBytes, 2 * img);
    if (rc) return rc;
    ORBX_HIP(hipMemcpyAsync(s->d_raw, left, span, hipMemcpyHostToDevice, h->stream));
    ORBX_HIP(hipMemcpyAsync(s->d_raw + img, right, span, hipMemcpyHostToDevice, h->stream));
    const uint8_t *pair;
    int gstride;
    size_t gimg;
    rc = rectify_pair(h, rl, rr, s->d_raw, s->d_raw + img, channels, rgb, w, hgt, stride, &pair, &gstride, &gimg);
    if (rc) return rc;
    return orbx_internal_stereo_frame_device(h, pair, w, hgt, gstride, gimg, mbf, mb, cap, kl, dl, nl, kr, dr, nr, uright, depth, nmatch);
}

extern "C" int orbx_stereo_frame_view_rectified(orbx_extractor_t *h, const orbx_rectifier_t *rl, const orbx_rectifier_t *rr,
                                                const uint8_t *left, const uint8_t *right, int channels, int rgb, int w, int hgt,
                                                int stride, float mbf, float mb, orbx_stereo_view_t *view) {
    if (!h || !view) { orbx_set_error("orbx_stereo_frame_view_rectified: bad arguments"); return ORBX_ERR_ARG; }
    memset(view, 0, sizeof(*view));
    if (bad_rect_args(h, rl, rr, channels, w, hgt, stride, "orbx_stereo_frame_view_rectified")) return ORBX_ERR_ARG;
    if (!left || !right || w <= 0 || hgt <= 0) return ORBX_OK;   // empty image
    ORBX_HIP(hipSetDevice(h->device));
    if (!h->rect) h->rect = new RectScratch();
    RectScratch *s = h->rect;
    const size_t span = (size_t)stride * (hgt - 1) + (size_t)w * channels, img = (span + 255) & ~(size_t)255;
    const uint8_t *dl = orbx_internal_device_visible(left), *dr = orbx_internal_device_visible(right);
    if (!dl || !dr) {   // pageable memory: one memcpy per image into pinned staging, which the remap reads over the bus
        if (s->stageBytes < 2 * img) {
            ORBX_HIP(hipStreamSynchronize(h->stream));
            if (s->h_stage) { hipHostFree(s->h_stage); s->h_stage = nullptr; s->stageBytes = 0; }
            ORBX_HIP(scratch_host_malloc((void **)&s->h_stage, 2 * img, hipHostMallocDefault));
            ORBX_HIP(hipHostGetDevicePointer((void **)&s->h_stage_dev, s->h_stage, 0));
            s->stageBytes = 2 * img;
        }
        if (!dl) { memcpy(s->h_stage, left, span); dl = s->h_stage_dev; }
        if (!dr) { memcpy(s->h_stage + img, right, span); dr = s->h_stage_dev + img; }
    }
    const uint8_t *pair;
    int gstride;
    size_t gimg;
    int rc = rectify_pair(h, rl, rr, dl, dr, channels, rgb, w, hgt, stride, &pair, &gstride, &gimg);
    if (rc) return rc;
    // the gray pair is device memory: the latency form reads it in place, behind the remap on the same stream
    return orbx_stereo_frame_view(h, pair, pair + gimg, w, hgt, gstride, mbf, mb, view);
}
