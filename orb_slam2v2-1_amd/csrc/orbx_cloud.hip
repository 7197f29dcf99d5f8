// orbx_cloud.hip — MI355X (gfx950) dense RGB-D keyframe clouds: hand-written HIP kernels + C ABI.
//
//   k_cloud_count / k_cloud_emit   PointCloudMapping::generatePointCloud (src/pointcloudmapping.cc:83-114): every step-th pixel of
//                                  every step-th row, GrabImageRGBD's depth conversion (src/Tracking.cc:335-336), the depth gate,
//                                  back-projection, pcl::transformPointCloud with a double 4x4, colour fetch - compacted in scan order
//   k_vox_*  / k_radix_*           pcl::VoxelGrid<PointXYZRGBA>::applyFilter (PCL 1.8, downsample_all_data) as saveOctomap runs it
//                                  (:117-127): finite-point extents, cell index, stable sort by cell, one centroid per cell
//   orbx_keyframe_cloud            one keyframe host to host
//
// Ordered compaction (orbx_cloud_dev.h) is used three times - valid samples, finite points, heads of the sorted runs - over per-frame
// tiles: grid (workgroups of a frame, B), frame b's elements at b * cap, k_cloud_scan the scan of a frame's counts.  The sort is that
// header's too, of (cell index, input index) pairs: its histogram is frame-major, [B][workgroups][256], scanned by one lane per digit
// (k_radix_scan), and the passes that run are the 8-bit digits of the batch's largest key (batchMax).
// The arithmetic is restated in DESIGN.md §3 and, in numpy, in tests/cloud_ref.py.
#include "orbx_cloud_dev.h"
#include <math.h>
#include <algorithm>

#define VE_FLIGHT 16                      // points k_vox_emit loads ahead of its sequential sums
#define CL_POSES 16                       // poses per launch of k_cloud_emit (kernel arguments: 16 x 12 doubles = 1.5 KB)

struct CloudPoses {
    double m[CL_POSES][12];   // rows 0..2 of Twc, row-major
};

struct GenArgs {
    const uint8_t *depth; size_t depthImg; int depthStride, depthType; float factor; int convert;
    const uint8_t *color; size_t colorImg; int colorStride, channels;
    int w, h, step, gw, ns;   // gw: samples per row, ns: samples per frame
    float fx, fy, cx, cy;
    int alpha;
};

// per-frame state of the voxel filter; everything between the kernels lives here, the host reads none of it
struct VoxMeta {
    uint32_t mn[3], mx[3];   // extents of the finite points as order-preserving integers (f2o)
    int32_t minb[3];
    uint32_t mul1, mul2;     // divb.x, divb.x * divb.y
    int32_t overflow;
};

__device__ __forceinline__ uint32_t f2o(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float o2f(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
// a word other workgroups update with atomics, as the L2 holds it now (a stale value only costs an atomic more)
__device__ __forceinline__ uint32_t peek(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Per-workgroup counts [B][nblk] -> exclusive offsets in place, the frame's total to tot[b].  One workgroup per frame.
// outCounts (may be NULL): min(total, clampCap), or -1 for a frame whose grid overflowed.
__global__ __launch_bounds__(CL_THREADS) void k_cloud_scan(int32_t *__restrict__ blk, int nblk, int32_t *__restrict__ tot,
                                                           int32_t *__restrict__ outCounts, int clampCap,
                                                           const VoxMeta *__restrict__ meta) {
    __shared__ int lds[4];
    const int b = blockIdx.x;
    const int total = scan_counts(blk + (size_t)b * nblk, nblk, lds);
    if (threadIdx.x == 0) {
        tot[b] = total;
        if (outCounts) outCounts[b] = (meta && meta[b].overflow) ? -1 : min(total, clampCap);
    }
}

// ---- generate

// mImDepth.at<float>(m, n) after GrabImageRGBD's conversion, and the gate `d < 0.01 || d > 10` with the float compared as double:
// NaN passes both comparisons and is kept
__device__ __forceinline__ bool cloud_sample(const GenArgs &a, int b, int s, float &d, int &m, int &n) {
    const int mi = s / a.gw;
    m = mi * a.step;
    n = (s - mi * a.gw) * a.step;
    const uint8_t *row = a.depth + (size_t)b * a.depthImg + (size_t)m * a.depthStride;
    if (a.depthType == ORBX_DEPTH_U16) d = (float)((const uint16_t *)row)[n] * a.factor;
    else {
        d = ((const float *)row)[n];
        if (a.convert) d = d * a.factor;
    }
    return !((double)d < 0.01 || (double)d > 10.0);
}

__global__ __launch_bounds__(CL_THREADS) void k_cloud_count(GenArgs a, int32_t *__restrict__ blk) {
    __shared__ int segs[CL_SEGS];
    const int b = blockIdx.y, base = blockIdx.x * CL_TILE;
    bool flag[CL_ITERS];
    int rank[CL_ITERS];
#pragma unroll
    for (int k = 0; k < CL_ITERS; k++) {
        const int s = tile_elem(base, k);
        float d; int m, n;
        flag[k] = s < a.ns && cloud_sample(a, b, s, d, m, n);
    }
    const int total = block_ranks(flag, rank, segs);
    if (threadIdx.x == 0) blk[(size_t)b * gridDim.x + blockIdx.x] = total;
}

// frames [b0, b0 + gridDim.y): poses.m[blockIdx.y] is frame b0 + blockIdx.y's
__global__ __launch_bounds__(CL_THREADS) void k_cloud_emit(GenArgs a, CloudPoses poses, int b0, const int32_t *__restrict__ blk, int nblk,
                                                          orbx_cloud_point_t *__restrict__ pts, int cap) {
    __shared__ int segs[CL_SEGS];
    const int b = b0 + blockIdx.y, base = blockIdx.x * CL_TILE;
    bool flag[CL_ITERS];
    int rank[CL_ITERS], pm[CL_ITERS], pn[CL_ITERS];
    float dep[CL_ITERS];
#pragma unroll
    for (int k = 0; k < CL_ITERS; k++) {
        const int s = tile_elem(base, k);
        dep[k] = 0.f; pm[k] = pn[k] = 0;
        flag[k] = s < a.ns && cloud_sample(a, b, s, dep[k], pm[k], pn[k]);
    }
    block_ranks(flag, rank, segs);
    const int off = blk[(size_t)b * nblk + blockIdx.x];
    const double *M = poses.m[blockIdx.y];
#pragma unroll
    for (int k = 0; k < CL_ITERS; k++) {
        const int r = off + rank[k];
        if (!flag[k] || r >= cap) continue;
        const float z = dep[k];
        const float x = ((float)pn[k] - a.cx) * z / a.fx;
        const float y = ((float)pm[k] - a.cy) * z / a.fy;
        const double xd = (double)x, yd = (double)y, zd = (double)z;
        orbx_cloud_point_t p;
        p.x = (float)(M[0] * xd + M[1] * yd + M[2] * zd + M[3]);
        p.y = (float)(M[4] * xd + M[5] * yd + M[6] * zd + M[7]);
        p.z = (float)(M[8] * xd + M[9] * yd + M[10] * zd + M[11]);
        const uint8_t *c = a.color + (size_t)b * a.colorImg + (size_t)pm[k] * a.colorStride + (size_t)pn[k] * a.channels;
        p.b = c[0]; p.g = c[1]; p.r = c[2];   // channel 0 is "b" whatever the capture's order (:99-101)
        p.a = (uint8_t)a.alpha;
        pts[(size_t)b * cap + r] = p;
    }
}

// ---- voxel grid

__global__ void k_vox_init(VoxMeta *__restrict__ meta, int B, uint32_t *__restrict__ batchMax) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0) *batchMax = 0u;
    if (b >= B) return;
    for (int k = 0; k < 3; k++) { meta[b].mn[k] = 0xffffffffu; meta[b].mx[k] = 0u; meta[b].minb[k] = 0; }
    meta[b].mul1 = meta[b].mul2 = 0u;
    meta[b].overflow = 0;
}

// finite points per workgroup, and their extents (integer atomic min / max at the L2: the result does not depend on the order)
__global__ __launch_bounds__(CL_THREADS) void k_vox_minmax(const orbx_cloud_point_t *__restrict__ pts, const int32_t *__restrict__ counts,
                                                          int cap, int32_t *__restrict__ blk, VoxMeta *__restrict__ meta) {
    __shared__ int segs[CL_SEGS];
    __shared__ uint32_t red[4][6];
    const int b = blockIdx.y, base = blockIdx.x * CL_TILE, n = frame_points(counts, b, cap);
    bool flag[CL_ITERS];
    int rank[CL_ITERS];
    uint32_t mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < CL_ITERS; k++) {
        const int i = tile_elem(base, k);
        flag[k] = false;
        if (i < n) {
            const orbx_cloud_point_t p = pts[(size_t)b * cap + i];
            if (finite_bits(p.x) && finite_bits(p.y) && finite_bits(p.z)) {
                flag[k] = true;
                const uint32_t o[3] = {f2o(p.x), f2o(p.y), f2o(p.z)};
#pragma unroll
                for (int c = 0; c < 3; c++) { mn[c] = min(mn[c], o[c]); mx[c] = max(mx[c], o[c]); }
            }
        }
    }
    const int total = block_ranks(flag, rank, segs);
    if (threadIdx.x == 0) blk[(size_t)b * gridDim.x + blockIdx.x] = total;
    if (total == 0) return;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        mn[c] = wave_reduce(mn[c], [](uint32_t x, uint32_t y) { return min(x, y); });
        mx[c] = wave_reduce(mx[c], [](uint32_t x, uint32_t y) { return max(x, y); });
    }
    // the four waves' extents meet in LDS: one atomic per word and workgroup (atomics on one word run one at a time at the L2)
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) { red[threadIdx.x >> 6][c] = mn[c]; red[threadIdx.x >> 6][3 + c] = mx[c]; }
    }
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(&meta[b].mn[threadIdx.x], min(min(red[0][threadIdx.x], red[1][threadIdx.x]), min(red[2][threadIdx.x], red[3][threadIdx.x])));
    else if (threadIdx.x < 6) atomicMax(&meta[b].mx[threadIdx.x - 3], max(max(red[0][threadIdx.x], red[1][threadIdx.x]), max(red[2][threadIdx.x], red[3][threadIdx.x])));
}

// extents -> overflow flag, min_b, div_b of every frame (applyFilter's head); one lane per frame
__global__ __launch_bounds__(CL_THREADS) void k_vox_grid(VoxMeta *__restrict__ meta, const int32_t *__restrict__ nfin, int B, float leaf) {
    const float inv = 1.0f / leaf;
    for (int b = blockIdx.x * CL_THREADS + threadIdx.x; b < B; b += gridDim.x * CL_THREADS) {
        if (nfin[b] <= 0) continue;
        VoxMeta &m = meta[b];
        bool ovf = false;
        long long d[3] = {1, 1, 1};
        int divb[3];
        for (int k = 0; k < 3; k++) {
            const float lo = o2f(m.mn[k]), hi = o2f(m.mx[k]);
            const float e = (hi - lo) * inv;
            if (!(e < 2147483648.0f)) ovf = true;   // an extent past int32 alone overflows the product (and the cast)
            else d[k] = (long long)e + 1;
            const int lb = (int)floorf(lo * inv), hb = (int)floorf(hi * inv);
            m.minb[k] = lb;
            divb[k] = hb - lb + 1;
        }
        if (!ovf) {
            const long long p = d[0] * d[1];
            if (p > 2147483647ll || p * d[2] > 2147483647ll) ovf = true;
        }
        m.mul1 = (uint32_t)divb[0];
        m.mul2 = (uint32_t)divb[0] * (uint32_t)divb[1];
        m.overflow = ovf ? 1 : 0;
    }
}

__device__ __forceinline__ int radix_digits(uint32_t m) {
    return m ? (32 - __clz(m) + 7) / 8 : 0;
}

// (cell index, input index) of every finite point, compacted in input order; batchMax: a cell index with as many
// 8-bit digits as the batch's largest
__global__ __launch_bounds__(CL_THREADS) void k_vox_keys(const orbx_cloud_point_t *__restrict__ pts, const int32_t *__restrict__ counts,
                                                        int cap, const int32_t *__restrict__ blk, const VoxMeta *__restrict__ meta,
                                                        float leaf, uint32_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                        uint32_t *__restrict__ batchMax) {
    __shared__ int segs[CL_SEGS];
    __shared__ uint32_t kred[4];
    const int b = blockIdx.y, base = blockIdx.x * CL_TILE, n = frame_points(counts, b, cap);
    if (meta[b].overflow || base >= n) return;   // (uniform over the workgroup)
    const float inv = 1.0f / leaf;
    const VoxMeta m = meta[b];
    bool flag[CL_ITERS];
    int rank[CL_ITERS];
    uint32_t key[CL_ITERS], kmax = 0u;
#pragma unroll
    for (int k = 0; k < CL_ITERS; k++) {
        const int i = tile_elem(base, k);
        flag[k] = false; key[k] = 0u;
        if (i < n) {
            const orbx_cloud_point_t p = pts[(size_t)b * cap + i];
            if (finite_bits(p.x) && finite_bits(p.y) && finite_bits(p.z)) {
                flag[k] = true;
                const int i0 = (int)(floorf(p.x * inv) - (float)m.minb[0]);
                const int i1 = (int)(floorf(p.y * inv) - (float)m.minb[1]);
                const int i2 = (int)(floorf(p.z * inv) - (float)m.minb[2]);
                key[k] = (uint32_t)i0 + (uint32_t)i1 * m.mul1 + (uint32_t)i2 * m.mul2;
                kmax = max(kmax, key[k]);
            }
        }
    }
    block_ranks(flag, rank, segs);
    const int off = blk[(size_t)b * gridDim.x + blockIdx.x];
#pragma unroll
    for (int k = 0; k < CL_ITERS; k++) {
        if (!flag[k]) continue;
        const size_t o = (size_t)b * cap + off + rank[k];
        keys[o] = key[k];
        vals[o] = (uint32_t)tile_elem(base, k);
    }
    kmax = wave_reduce(kmax, [](uint32_t x, uint32_t y) { return max(x, y); });
    if ((threadIdx.x & 63) == 0) kred[threadIdx.x >> 6] = kmax;
    __syncthreads();
    // only the number of 8-bit digits matters: a workgroup sends its key only if that has more of them than the word holds
    if (threadIdx.x == 0) {
        kmax = max(max(kred[0], kred[1]), max(kred[2], kred[3]));
        if (radix_digits(kmax) > radix_digits(peek(batchMax))) atomicMax(batchMax, kmax);
    }
}

// The sort of (key, value) by key, every frame of the batch in one launch.  Pass p runs only while the batch's largest key has bits
// at or above 8p (batchMax, read on the device); it reads buffer p & 1 and writes the other, so after the passes that ran the
// sorted pairs sit in buffer (passes & 1).
__device__ __forceinline__ int sort_points(const VoxMeta *meta, const int32_t *nfin, int b) {
    return meta[b].overflow ? 0 : nfin[b];
}

__global__ __launch_bounds__(CL_THREADS) void k_radix_hist(int pass, const uint32_t *__restrict__ keys2, size_t N, int cap,
                                                          const VoxMeta *__restrict__ meta, const int32_t *__restrict__ nfin,
                                                          const uint32_t *__restrict__ batchMax, uint32_t *__restrict__ hist) {
    __shared__ uint32_t h[256];
    if (pass >= radix_digits(*batchMax)) return;
    const int b = blockIdx.y, base = blockIdx.x * CL_TILE, n = sort_points(meta, nfin, b);
    if (base >= n) return;
    const uint32_t *keys = keys2 + (size_t)(pass & 1) * N + (size_t)b * cap;
    radix_tile_hist(keys, n, base, pass, h);
    hist[((size_t)b * gridDim.x + blockIdx.x) * 256 + threadIdx.x] = h[threadIdx.x];
}

// hist [B][nblk][256] -> for digit d (one lane each): the running count over the frame's workgroups in place, and the digit's
// first position to digitBase [B][256]
__global__ __launch_bounds__(CL_THREADS) void k_radix_scan(int pass, int nblk, const VoxMeta *__restrict__ meta,
                                                          const int32_t *__restrict__ nfin, const uint32_t *__restrict__ batchMax,
                                                          uint32_t *__restrict__ hist, uint32_t *__restrict__ digitBase) {
    __shared__ int lds[4];
    if (pass >= radix_digits(*batchMax)) return;
    const int b = blockIdx.x, n = sort_points(meta, nfin, b);
    const int nact = (n + CL_TILE - 1) / CL_TILE;
    uint32_t *h = hist + (size_t)b * nblk * 256 + threadIdx.x;
    uint32_t run = 0u;
    for (int i = 0; i < nact; i++) {
        const uint32_t v = h[(size_t)i * 256];
        h[(size_t)i * 256] = run;
        run += v;
    }
    int total;
    digitBase[(size_t)b * 256 + threadIdx.x] = (uint32_t)block_excl_scan((int)run, lds, total);
}

__global__ __launch_bounds__(CL_THREADS) void k_radix_scatter(int pass, uint32_t *__restrict__ keys2, uint32_t *__restrict__ vals2, size_t N,
                                                             int cap, const VoxMeta *__restrict__ meta, const int32_t *__restrict__ nfin,
                                                             const uint32_t *__restrict__ batchMax, const uint32_t *__restrict__ hist,
                                                             const uint32_t *__restrict__ digitBase) {
    __shared__ uint32_t seg[CL_SEGS][256];   // [segment][digit]: count, then first position
    if (pass >= radix_digits(*batchMax)) return;
    const int b = blockIdx.y, base = blockIdx.x * CL_TILE, n = sort_points(meta, nfin, b);
    if (base >= n) return;
    const size_t src = (size_t)(pass & 1) * N + (size_t)b * cap, dst = (size_t)((pass + 1) & 1) * N + (size_t)b * cap;
    for (int s = 0; s < CL_SEGS; s++) seg[s][threadIdx.x] = 0u;
    __syncthreads();
    uint32_t key[CL_ITERS], val[CL_ITERS];
    bool flag[CL_ITERS];
#pragma unroll
    for (int k = 0; k < CL_ITERS; k++) {
        const int i = tile_elem(base, k);
        flag[k] = i < n;
        key[k] = flag[k] ? keys2[src + i] : 0u;
        val[k] = flag[k] ? vals2[src + i] : 0u;
    }
    radix_tile_scatter(
        key, flag, pass, n, seg,
        [&] { return digitBase[(size_t)b * 256 + threadIdx.x] + hist[((size_t)b * gridDim.x + blockIdx.x) * 256 + threadIdx.x]; },
        [&](int k, uint32_t o) { keys2[dst + o] = key[k]; vals2[dst + o] = val[k]; });
}

// heads of the runs of equal keys, per workgroup
__global__ __launch_bounds__(CL_THREADS) void k_vox_heads(const uint32_t *__restrict__ keys2, size_t N, int cap,
                                                         const VoxMeta *__restrict__ meta, const int32_t *__restrict__ nfin,
                                                         const uint32_t *__restrict__ batchMax, int32_t *__restrict__ blk) {
    __shared__ int segs[CL_SEGS];
    const int b = blockIdx.y, base = blockIdx.x * CL_TILE, n = sort_points(meta, nfin, b);
    const uint32_t *keys = keys2 + (size_t)(radix_digits(*batchMax) & 1) * N + (size_t)b * cap;
    bool flag[CL_ITERS];
    int rank[CL_ITERS];
    run_heads(keys, n, base, flag);
    const int total = block_ranks(flag, rank, segs);
    if (threadIdx.x == 0) blk[(size_t)b * gridDim.x + blockIdx.x] = total;
}

// One lane per voxel - the lane of the run's head: x, y, z and the four colour bytes summed sequentially in float in the run's order
// (ascending input index: the sort is stable), divided by (float)count; the colour quotient is truncated.
__global__ __launch_bounds__(CL_THREADS) void k_vox_emit(const orbx_cloud_point_t *__restrict__ pts, const uint32_t *__restrict__ keys2,
                                                        const uint32_t *__restrict__ vals2, size_t N, int cap,
                                                        const VoxMeta *__restrict__ meta, const int32_t *__restrict__ nfin,
                                                        const uint32_t *__restrict__ batchMax, const int32_t *__restrict__ blk,
                                                        orbx_cloud_point_t *__restrict__ out, int outCap) {
    __shared__ int segs[CL_SEGS];
    const int b = blockIdx.y, base = blockIdx.x * CL_TILE, n = sort_points(meta, nfin, b);
    if (base >= n) return;
    const size_t o = (size_t)(radix_digits(*batchMax) & 1) * N + (size_t)b * cap;
    const uint32_t *keys = keys2 + o, *vals = vals2 + o;
    bool flag[CL_ITERS];
    int rank[CL_ITERS];
    run_heads(keys, n, base, flag);
    block_ranks(flag, rank, segs);
    const int off = blk[(size_t)b * gridDim.x + blockIdx.x];
    for (int k = 0; k < CL_ITERS; k++) {
        const int r = off + rank[k];
        if (!flag[k] || r >= outCap) continue;
        const int i = tile_elem(base, k);
        const uint32_t key = keys[i];
        // the run's end: the keys are sorted, so a doubling search and a bisection find it in O(log length) dependent loads
        int lo = i, stride = 1;
        while (lo + stride < n && keys[lo + stride] == key) { lo += stride; stride <<= 1; }
        int e = min(lo + stride, n);
        while (e - lo > 1) {
            const int mid = (lo + e) >> 1;
            if (keys[mid] == key) lo = mid; else e = mid;
        }
        // VE_FLIGHT points in flight at a time (a run is one lane's chain of dependent loads); the additions stay in the run's order
        float sx = 0.f, sy = 0.f, sz = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sa = 0.f;
        for (int j = i; j < e; j += VE_FLIGHT) {
            uint32_t src[VE_FLIGHT];
            orbx_cloud_point_t p[VE_FLIGHT];
#pragma unroll
            for (int u = 0; u < VE_FLIGHT; u++) src[u] = j + u < e ? vals[j + u] : 0u;
#pragma unroll
            for (int u = 0; u < VE_FLIGHT; u++) p[u] = pts[(size_t)b * cap + min(src[u], (uint32_t)cap - 1u)];   // (min: kept as the load's bound)
#pragma unroll
            for (int u = 0; u < VE_FLIGHT; u++) {
                if (j + u < e) {
                    sx += p[u].x; sy += p[u].y; sz += p[u].z;
                    sr += (float)p[u].r; sg += (float)p[u].g; sb += (float)p[u].b; sa += (float)p[u].a;
                }
            }
        }
        const int cnt = e - i;
        const float c = (float)cnt;
        orbx_cloud_point_t q;
        q.x = sx / c; q.y = sy / c; q.z = sz / c;
        q.r = (uint8_t)(uint32_t)(sr / c); q.g = (uint8_t)(uint32_t)(sg / c);
        q.b = (uint8_t)(uint32_t)(sb / c); q.a = (uint8_t)(uint32_t)(sa / c);
        out[(size_t)b * outCap + r] = q;
    }
}

// ---- host side (the mapper handle: orbx_cloud_dev.h)

extern "C" int orbx_cloudmapper_create(float leaf, int step, int alpha, int device, orbx_cloudmapper_t **out) {
    if (!out || !(leaf > 0.0f) || !(leaf < INFINITY) || step < 1 || alpha < 0 || alpha > 255 || device < 0) {
        orbx_set_error("orbx_cloudmapper_create: bad arguments (leaf > 0, step >= 1, alpha 0..255, out != NULL)");
        return ORBX_ERR_ARG;
    }
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        (void)hipGetLastError();
        orbx_set_error("no usable HIP device");
        return ORBX_ERR_NO_DEVICE;
    }
    if (device >= ndev) {
        orbx_set_error("orbx_cloudmapper_create: device %d of %d", device, ndev);
        return ORBX_ERR_ARG;
    }
    ORBX_HIP(hipSetDevice(device));
    orbx_cloudmapper *m = new orbx_cloudmapper();   // (zero-initialised)
    m->leaf = leaf; m->step = step; m->alpha = alpha; m->device = device;
    hipError_t e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete m;
        ORBX_HIP(e);
    }
    *out = m;
    return ORBX_OK;
}

extern "C" int orbx_cloudmapper_destroy(orbx_cloudmapper_t *m) {
    if (!m) return ORBX_OK;
    hipSetDevice(m->device);
    if (m->stream) { hipStreamSynchronize(m->stream); hipStreamDestroy(m->stream); }
    hipFree(m->d_blk); hipFree(m->d_tot); hipFree(m->d_meta); hipFree(m->d_pairs); hipFree(m->d_hist); hipFree(m->d_digit);
    hipFree(m->d_octCodes); hipFree(m->d_octBlk); hipFree(m->d_octHist); hipFree(m->d_octState);
    hipFree(m->d_color); hipFree(m->d_depth); hipFree(m->d_raw); hipFree(m->d_out); hipFree(m->d_cnt);
    delete m;
    return ORBX_OK;
}

extern "C" int orbx_cloud_capacity(int w, int hgt, int step) {
    if (w < 1 || hgt < 1 || step < 1) return 0;
    const long long c = (long long)((w + step - 1) / step) * ((hgt + step - 1) / step);
    return c > 2147483647ll ? -1 : (int)c;
}

static size_t depth_esize(int t) { return t == ORBX_DEPTH_U16 ? 2 : 4; }

static int launch_generate(orbx_cloudmapper *m, const void *d_depth, int depth_type, int depth_stride, size_t depth_image_stride,
                           float factor, const uint8_t *d_color, int channels, int color_stride, size_t color_image_stride, int B, int w,
                           int hgt, float fx, float fy, float cx, float cy, const double *Twc16, orbx_cloud_point_t *d_points, int cap,
                           int32_t *d_counts, hipStream_t st) {
    GenArgs a;
    a.depth = (const uint8_t *)d_depth; a.depthImg = depth_image_stride; a.depthStride = depth_stride; a.depthType = depth_type;
    a.factor = factor;
    a.convert = (fabs(factor - 1.0f) > 1e-5 || depth_type != ORBX_DEPTH_F32) ? 1 : 0;   // src/Tracking.cc:335-336
    a.color = d_color; a.colorImg = color_image_stride; a.colorStride = color_stride; a.channels = channels;
    a.w = w; a.h = hgt; a.step = m->step; a.gw = (w + m->step - 1) / m->step;
    a.ns = orbx_cloud_capacity(w, hgt, m->step);
    a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.alpha = m->alpha;
    const int nblk = (a.ns + CL_TILE - 1) / CL_TILE;
    int rc = reserve(&m->d_blk, &m->blkBytes, sizeof(int32_t) * (size_t)B * nblk);
    if (!rc) rc = reserve(&m->d_tot, &m->totBytes, sizeof(int32_t) * (size_t)B);
    if (rc) return rc;
    int32_t *blk = (int32_t *)m->d_blk;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_cloud_count, dim3(nblk, B), dim3(CL_THREADS), 0, st, a, blk);
    hipLaunchKernelGGL(k_cloud_scan, dim3(B), dim3(CL_THREADS), 0, st, blk, nblk, (int32_t *)m->d_tot, d_counts, cap, (const VoxMeta *)nullptr);
    for (int b0 = 0; b0 < B; b0 += CL_POSES) {   // the poses travel as kernel arguments: no copy command on the stream
        const int nb = std::min(CL_POSES, B - b0);
        CloudPoses P;
        memset(&P, 0, sizeof(P));
        for (int i = 0; i < nb; i++) memcpy(P.m[i], Twc16 + (size_t)(b0 + i) * 16, sizeof(double) * 12);
        hipLaunchKernelGGL(k_cloud_emit, dim3(nblk, nb), dim3(CL_THREADS), 0, st, a, P, b0, (const int32_t *)blk, nblk, d_points, cap);
    }
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbx_cloud_generate_device(orbx_cloudmapper_t *m, const void *d_depth, int depth_type, int depth_stride,
                                          size_t depth_image_stride_bytes, float depth_map_factor, const uint8_t *d_color, int channels,
                                          int color_stride, size_t color_image_stride_bytes, int B, int w, int hgt, float fx, float fy,
                                          float cx, float cy, const double *Twc16, orbx_cloud_point_t *d_points, int cap,
                                          int32_t *d_counts, void *stream) {
    const size_t es = depth_esize(depth_type);
    if (!m || !d_depth || !d_color || !Twc16 || !d_points || !d_counts || B < 1 || B > 65535 || w < 1 || hgt < 1 || cap < 1 ||
        (depth_type != ORBX_DEPTH_U16 && depth_type != ORBX_DEPTH_F32) || (channels != 3 && channels != 4) ||
        depth_stride < 0 || (size_t)depth_stride < (size_t)w * es || (depth_stride & (es - 1)) || ((uintptr_t)d_depth & (es - 1)) ||
        (depth_image_stride_bytes & (es - 1)) || color_stride < 0 || (size_t)color_stride < (size_t)w * channels ||
        (B > 1 && (depth_image_stride_bytes < (size_t)depth_stride * hgt || color_image_stride_bytes < (size_t)color_stride * hgt)) ||
        ((uintptr_t)d_points & 3) || orbx_cloud_capacity(w, hgt, m->step) < 1 || !(fx != 0.0f) || !(fy != 0.0f)) {
        orbx_set_error("orbx_cloud_generate_device: bad arguments");
        return ORBX_ERR_ARG;
    }
    ORBX_HIP(hipSetDevice(m->device));
    return launch_generate(m, d_depth, depth_type, depth_stride, depth_image_stride_bytes, depth_map_factor, d_color, channels,
                           color_stride, color_image_stride_bytes, B, w, hgt, fx, fy, cx, cy, Twc16, d_points, cap, d_counts,
                           (hipStream_t)stream);
}

static int launch_voxel(orbx_cloudmapper *m, const orbx_cloud_point_t *d_points, const int32_t *d_counts, int B, int cap,
                        orbx_cloud_point_t *d_out, int out_cap, int32_t *d_out_counts, hipStream_t st) {
    const int nblk = (cap + CL_TILE - 1) / CL_TILE;
    const size_t N = (size_t)B * cap;
    int rc = reserve(&m->d_blk, &m->blkBytes, sizeof(int32_t) * (size_t)B * nblk);
    if (!rc) rc = reserve(&m->d_tot, &m->totBytes, sizeof(int32_t) * 2 * (size_t)B);
    if (!rc) rc = reserve(&m->d_meta, &m->metaBytes, sizeof(VoxMeta) * (size_t)B + 16);
    if (!rc) rc = reserve(&m->d_pairs, &m->pairBytes, sizeof(uint32_t) * 4 * N);
    if (!rc) rc = reserve(&m->d_hist, &m->histBytes, sizeof(uint32_t) * 256 * (size_t)B * nblk);
    if (!rc) rc = reserve(&m->d_digit, &m->digitBytes, sizeof(uint32_t) * 256 * (size_t)B);
    if (rc) return rc;
    int32_t *blk = (int32_t *)m->d_blk, *tot = (int32_t *)m->d_tot;
    VoxMeta *meta = (VoxMeta *)m->d_meta;
    uint32_t *batchMax = (uint32_t *)(m->d_meta + sizeof(VoxMeta) * (size_t)B);
    uint32_t *keys = (uint32_t *)m->d_pairs, *vals = keys + 2 * N;
    uint32_t *hist = (uint32_t *)m->d_hist, *digit = (uint32_t *)m->d_digit;
    const dim3 grid(nblk, B), block(CL_THREADS);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_vox_init, dim3((B + 255) / 256), dim3(256), 0, st, meta, B, batchMax);
    hipLaunchKernelGGL(k_vox_minmax, grid, block, 0, st, d_points, d_counts, cap, blk, meta);
    hipLaunchKernelGGL(k_cloud_scan, dim3(B), block, 0, st, blk, nblk, tot, (int32_t *)nullptr, 0, (const VoxMeta *)nullptr);
    hipLaunchKernelGGL(k_vox_grid, dim3(std::min((B + CL_THREADS - 1) / CL_THREADS, 256)), block, 0, st, meta, (const int32_t *)tot, B, m->leaf);
    hipLaunchKernelGGL(k_vox_keys, grid, block, 0, st, d_points, d_counts, cap, (const int32_t *)blk, (const VoxMeta *)meta, m->leaf, keys,
                       vals, batchMax);
    for (int p = 0; p < 4; p++) {
        hipLaunchKernelGGL(k_radix_hist, grid, block, 0, st, p, (const uint32_t *)keys, N, cap, (const VoxMeta *)meta, (const int32_t *)tot,
                           (const uint32_t *)batchMax, hist);
        hipLaunchKernelGGL(k_radix_scan, dim3(B), block, 0, st, p, nblk, (const VoxMeta *)meta, (const int32_t *)tot,
                           (const uint32_t *)batchMax, hist, digit);
        hipLaunchKernelGGL(k_radix_scatter, grid, block, 0, st, p, keys, vals, N, cap, (const VoxMeta *)meta, (const int32_t *)tot,
                           (const uint32_t *)batchMax, (const uint32_t *)hist, (const uint32_t *)digit);
    }
    // (the finite counts stay in tot for k_vox_emit: the heads' totals go to a second row of it)
    hipLaunchKernelGGL(k_vox_heads, grid, block, 0, st, (const uint32_t *)keys, N, cap, (const VoxMeta *)meta, (const int32_t *)tot,
                       (const uint32_t *)batchMax, blk);
    hipLaunchKernelGGL(k_cloud_scan, dim3(B), block, 0, st, blk, nblk, tot + B, d_out_counts, out_cap, (const VoxMeta *)meta);
    hipLaunchKernelGGL(k_vox_emit, grid, block, 0, st, d_points, (const uint32_t *)keys, (const uint32_t *)vals, N, cap,
                       (const VoxMeta *)meta, (const int32_t *)tot, (const uint32_t *)batchMax, (const int32_t *)blk, d_out, out_cap);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbx_cloud_voxel_device(orbx_cloudmapper_t *m, const orbx_cloud_point_t *d_points, const int32_t *d_counts, int B,
                                       int cap, orbx_cloud_point_t *d_out, int out_cap, int32_t *d_out_counts, void *stream) {
    if (!m || !d_points || !d_counts || !d_out || !d_out_counts || B < 1 || B > 65535 || cap < 1 || out_cap < 1 ||
        ((uintptr_t)d_points & 3) || ((uintptr_t)d_out & 3) || (const void *)d_points == (const void *)d_out) {
        orbx_set_error("orbx_cloud_voxel_device: bad arguments");
        return ORBX_ERR_ARG;
    }
    ORBX_HIP(hipSetDevice(m->device));
    return launch_voxel(m, d_points, d_counts, B, cap, d_out, out_cap, d_out_counts, (hipStream_t)stream);
}

extern "C" int orbx_keyframe_cloud(orbx_cloudmapper_t *m, const uint8_t *color, int channels, int color_stride, const void *depth,
                                   int depth_type, int depth_stride, float depth_map_factor, int w, int hgt, float fx, float fy,
                                   float cx, float cy, const double *Twc16, int cap, orbx_cloud_point_t *raw_out, int *n_raw,
                                   orbx_cloud_point_t *out, int *n) {
    if (!m || !n || !out || !Twc16 || cap < 0 || (channels != 3 && channels != 4) ||
        (depth_type != ORBX_DEPTH_U16 && depth_type != ORBX_DEPTH_F32) || !(fx != 0.0f) || !(fy != 0.0f)) {
        orbx_set_error("orbx_keyframe_cloud: bad arguments");
        return ORBX_ERR_ARG;
    }
    *n = 0;
    if (n_raw) *n_raw = 0;
    if (!color || !depth || w <= 0 || hgt <= 0) return ORBX_OK;   // empty image: an empty cloud
    const size_t es = depth_esize(depth_type);
    if (color_stride < 0 || (size_t)color_stride < (size_t)w * channels || depth_stride < 0 || (size_t)depth_stride < (size_t)w * es ||
        (depth_stride & (es - 1))) {
        orbx_set_error("orbx_keyframe_cloud: bad stride");
        return ORBX_ERR_ARG;
    }
    const int full = orbx_cloud_capacity(w, hgt, m->step);
    if (full < 1) { orbx_set_error("orbx_keyframe_cloud: image too large"); return ORBX_ERR_ARG; }
    ORBX_HIP(hipSetDevice(m->device));
    const size_t cspan = (size_t)color_stride * (hgt - 1) + (size_t)w * channels, dspan = (size_t)depth_stride * (hgt - 1) + (size_t)w * es;
    int rc = reserve(&m->d_color, &m->colorBytes, cspan);
    if (!rc) rc = reserve(&m->d_depth, &m->depthBytes, dspan);
    if (!rc) rc = reserve(&m->d_raw, &m->rawBytes, sizeof(orbx_cloud_point_t) * (size_t)full);
    if (!rc) rc = reserve(&m->d_out, &m->outBytes, sizeof(orbx_cloud_point_t) * (size_t)full);
    if (!rc) rc = reserve(&m->d_cnt, &m->cntBytes, 2 * sizeof(int32_t));
    if (rc) return rc;
    hipStream_t st = m->stream;
    orbx_cloud_point_t *d_raw = (orbx_cloud_point_t *)m->d_raw, *d_out = (orbx_cloud_point_t *)m->d_out;
    int32_t *d_cnt = (int32_t *)m->d_cnt;
    ORBX_HIP(hipMemcpyAsync(m->d_color, color, cspan, hipMemcpyHostToDevice, st));
    ORBX_HIP(hipMemcpyAsync(m->d_depth, depth, dspan, hipMemcpyHostToDevice, st));
    rc = launch_generate(m, m->d_depth, depth_type, depth_stride, 0, depth_map_factor, m->d_color, channels, color_stride, 0, 1, w, hgt,
                         fx, fy, cx, cy, Twc16, d_raw, full, d_cnt, st);
    if (!rc) rc = launch_voxel(m, d_raw, d_cnt, 1, full, d_out, full, d_cnt + 1, st);
    if (rc) return rc;
    int32_t cnt[2] = {0, 0};
    ORBX_HIP(hipMemcpyAsync(cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    int status = ORBX_OK;
    int nr = cnt[0], nv = cnt[1];
    const bool unfiltered = nv < 0;   // the grid overflowed: VoxelGrid warns and hands its input on
    if (unfiltered) nv = nr;
    if (nr > cap || nv > cap) {
        orbx_set_error("keyframe cloud of %d raw / %d filtered points, cap %d", nr, nv, cap);
        status = ORBX_ERR_CAPACITY;
    }
    nr = std::min(nr, cap); nv = std::min(nv, cap);
    if (raw_out && nr > 0) ORBX_HIP(hipMemcpyAsync(raw_out, d_raw, sizeof(orbx_cloud_point_t) * (size_t)nr, hipMemcpyDeviceToHost, st));
    if (nv > 0) ORBX_HIP(hipMemcpyAsync(out, unfiltered ? d_raw : d_out, sizeof(orbx_cloud_point_t) * (size_t)nv, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    if (n_raw) *n_raw = nr;
    *n = nv;
    return status;
}
