// orbx_cloud_dev.h — what the dense-map sources share (orbx_cloud.hip: keyframe clouds and the voxel filter; orbx_octomap.hip: the
// occupancy octree): the tile geometry, ordered compaction, the radix sort's core and the mapper handle with its grow-only scratch.
//
// Ordered compaction.  A workgroup of 256 lanes owns a tile of 1024 consecutive elements as 16 wave-sized segments.  A ballot +
// popcount ranks a lane among the flagged lanes of its segment and the 16 segment counts meet in LDS (block_ranks).  A counting
// launch stores one count per workgroup, a scan launch of one workgroup per array turns the counts into offsets (scan_counts), and
// the writing launch repeats the ballots and stores at offset + rank.  No atomic decides a position, so the order is the input's;
// the price is that the predicate is evaluated twice.  (A single-launch chained scan would need workgroups to wait for each other.)
//
// The sort is an LSD radix sort, 8 bits a pass, between two buffers: per pass a histogram launch (radix_tile_hist: one 256-bin
// histogram per tile), a scan launch that turns the histograms into each tile's first position of each digit, and a scatter launch
// (radix_tile_scatter).  The scatter is ordered compaction per digit: eight ballots rank a lane among the lanes of its segment with
// the same digit, lane d of the workgroup walks the 16 segment counts of digit d on from the tile's first position, and an element
// lands at its segment's first position + its rank.  So a pass keeps equal digits in input order and the sort is stable, which is what
// lets k_vox_emit sum a voxel in input order.  What differs between the two users - the key type and payload, the layout of the
// histogram and its scan, which passes run and which buffer holds the result - stays in their kernels.
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
// this lane's element of iteration k in the tile that starts at base
__device__ __forceinline__ int tile_elem(int base, int k) {
    return base + k * CL_THREADS + threadIdx.x;
}

// Ranks of the workgroup's elements: flag[k] of element tile_elem(base, k) -> rank[k] among the flagged elements of the workgroup,
// in element order; returns the workgroup's count.  segs: CL_SEGS ints of LDS.
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

// counts c[0..nact) -> exclusive offsets in place, by the whole workgroup, 256 at a time with a carry; returns the total.  lds: 4 ints
__device__ __forceinline__ int scan_counts(int32_t *c, int nact, int *lds) {
    int carry = 0;
    for (int i0 = 0; i0 < nact; i0 += CL_THREADS) {
        const int i = i0 + threadIdx.x;
        const int v = i < nact ? c[i] : 0;
        int total;
        const int ex = block_excl_scan(v, lds, total);
        if (i < nact) c[i] = carry + ex;
        carry += total;
    }
    return carry;
}

// flag[k]: element tile_elem(base, k) heads a run of equal keys in the sorted keys[0..n)
template <typename K>
__device__ __forceinline__ void run_heads(const K *__restrict__ keys, int n, int base, bool (&flag)[CL_ITERS]) {
#pragma unroll
    for (int k = 0; k < CL_ITERS; k++) {
        const int i = tile_elem(base, k);
        flag[k] = i < n && (i == 0 || keys[i] != keys[i - 1]);
    }
}

// op over the 64 lanes of the wave, the result in every lane (op: associative and commutative)
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    return v;
}

template <typename K>
__device__ __forceinline__ uint32_t radix_digit(K key, int pass) {
    return (uint32_t)(key >> (8 * pass)) & 255u;
}

// h[d]: the tile's elements (of keys[0..n)) whose digit of this pass is d.  h: 256 words of LDS, complete on return
template <typename K>
__device__ __forceinline__ void radix_tile_hist(const K *__restrict__ keys, int n, int base, int pass, uint32_t *h) {
    h[threadIdx.x] = 0u;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CL_ITERS; k++) {
        const int i = tile_elem(base, k);
        if (i < n) atomicAdd(&h[radix_digit(keys[i], pass)], 1u);
    }
    __syncthreads();
}

// One pass's scatter of a tile: key[k] / flag[k] of element tile_elem(base, k).  seg: [segment][digit] in LDS, zero on entry (and
// published by a barrier).  first(): lane d's first position of digit d for this tile; put(k, o): store element k at position o < n.
template <typename K, typename First, typename Put>
__device__ __forceinline__ void radix_tile_scatter(const K (&key)[CL_ITERS], const bool (&flag)[CL_ITERS], int pass, int n,
                                                   uint32_t (*seg)[256], First first, Put put) {
    const int wv = threadIdx.x >> 6;
    int rank[CL_ITERS];
#pragma unroll
    for (int k = 0; k < CL_ITERS; k++) {
        const uint32_t d = radix_digit(key[k], pass);
        uint64_t same = __ballot(flag[k]);   // the segment's lanes with this lane's digit
#pragma unroll
        for (int bit = 0; bit < 8; bit++) {
            const bool one = (d >> bit) & 1u;
            const uint64_t m = __ballot(one);
            same &= one ? m : ~m;
        }
        rank[k] = __popcll(same & lanes_below());
        if (flag[k] && rank[k] == 0) seg[k * 4 + wv][d] = (uint32_t)__popcll(same);
    }
    __syncthreads();
    {   // lane d: count -> first position of digit d for every segment, in segment order
        uint32_t run = first();
        for (int s = 0; s < CL_SEGS; s++) {
            const uint32_t c = seg[s][threadIdx.x];
            seg[s][threadIdx.x] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CL_ITERS; k++) {
        if (!flag[k]) continue;
        const uint32_t o = seg[k * 4 + wv][radix_digit(key[k], pass)] + (uint32_t)rank[k];
        if (o < (uint32_t)n) put(k, o);   // (always: kept as the store's bound)
    }
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
    ORBX_HIP(scratch_malloc(p, need));
    *have = need;
    return ORBX_OK;
}
