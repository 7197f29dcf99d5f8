// orbx_cloud_dev.h — what the dense-map sources share (orbx_cloud.hip: keyframe clouds and the voxel filter; orbx_octomap.hip: the
// occupancy octree): the tile geometry, the ordered-compaction device helpers and the mapper handle with its grow-only scratch.
#pragma once
#include "orbx_internal.h"

#define CL_THREADS 256
#define CL_ITERS 4
#define CL_TILE (CL_THREADS * CL_ITERS)   // elements per workgroup
#define CL_SEGS (CL_TILE / 64)            // wave-sized segments per workgroup, in element order: segment = iteration * 4 + wave

__device__ __forceinline__ bool finite_bits(float f) {
    return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u;
}
__device__ __forceinline__ uint64_t lanes_below() {
    return (1ull << (threadIdx.x & 63)) - 1ull;
}

// Ranks of the workgroup's elements: flag[k] of iteration k (element base + k * 256 + threadIdx.x) -> rank[k] among the flagged
// elements of the workgroup, in element order; returns the workgroup's count.  segs: CL_SEGS ints of LDS.
__device__ __forceinline__ int block_ranks(const bool (&flag)[CL_ITERS], int (&rank)[CL_ITERS], int *segs) {
    const int wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < CL_ITERS; k++) {
        const uint64_t m = __ballot(flag[k]);
        rank[k] = __popcll(m & lanes_below());
        if ((threadIdx.x & 63) == 0) segs[k * 4 + wv] = __popcll(m);
    }
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int s = 0; s < CL_SEGS; s++) {
        const int c = segs[s];
#pragma unroll
        for (int k = 0; k < CL_ITERS; k++)
            if (s < k * 4 + wv) rank[k] += c;
        total += c;
    }
    __syncthreads();
    return total;
}

// exclusive scan of one value per lane over the 256 lanes; lds: 4 ints
__device__ __forceinline__ int block_excl_scan(int v, int *lds, int &total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) lds[wv] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (i < wv) base += lds[i];
        total += lds[i];
    }
    __syncthreads();
    return base + inc - v;
}

__device__ __forceinline__ int frame_points(const int32_t *counts, int b, int cap) {
    return min(max(counts[b], 0), cap);
}

struct orbx_cloudmapper {
    float leaf; int step, alpha, device;
    // grow-only scratch of the device calls (one stream at a time uses a mapper)
    uint8_t *d_blk; size_t blkBytes;       // int32 [B][workgroups]: counts, then offsets
    uint8_t *d_tot; size_t totBytes;       // int32 [2][B]: valid samples / finite points, voxels
    uint8_t *d_meta; size_t metaBytes;     // VoxMeta [B] + the batch's largest key
    uint8_t *d_pairs; size_t pairBytes;    // uint32 keys [2][B * cap] | values [2][B * cap]
    uint8_t *d_hist; size_t histBytes;     // uint32 [B][workgroups][256]
    uint8_t *d_digit; size_t digitBytes;   // uint32 [B][256]
    // orbx_octree_device (orbx_octomap.hip)
    uint8_t *d_octCodes; size_t octCodeBytes;   // uint64 [2][B * cap]: the radix sort's two buffers; then sorted codes | unique codes
    uint8_t *d_octBlk; size_t octBlkBytes;      // int32 [2][workgroups]: counts, then offsets
    uint8_t *d_octHist; size_t octHistBytes;    // uint32 [256][workgroups] + [256]
    uint8_t *d_octState; size_t octStateBytes;  // OctState
    // orbx_keyframe_cloud / orbx_octomap_bt
    hipStream_t stream;
    uint8_t *d_color; size_t colorBytes;
    uint8_t *d_depth; size_t depthBytes;
    uint8_t *d_raw; size_t rawBytes;
    uint8_t *d_out; size_t outBytes;
    uint8_t *d_cnt; size_t cntBytes;
};

static inline int reserve(uint8_t **p, size_t *have, size_t need) {
    need = ((need + 255) & ~(size_t)255) + 256;
    if (*have >= need) return ORBX_OK;
    hipFree(*p); *p = nullptr; *have = 0;   // (hipFree waits for the device: no kernel still reads the old block)
    ORBX_HIP(hipMalloc(p, need));
    *have = need;
    return ORBX_OK;
}
