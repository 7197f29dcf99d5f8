// orbx_octomap.hip — MI355X (gfx950) occupancy octree of the dense map: what PointCloudMapping::saveOctomap writes with
// octomap::OcTree::writeBinary (src/pointcloudmapping.cc:198-278), as hand-written HIP kernels + C ABI.  DESIGN.md §3 items 14-15,
// restated in plain Python in tests/octomap_ref.py.
//
//   k_oct_keys_*      pcl::transformPointCloud with a float 4x4, OcTreeKey of every point (coordToKeyChecked), the 48-bit preorder
//                     code of its depth-16 cell; invalid points compacted away in input order
//   k_oct_hist / k_oct_hscan / k_oct_scatter   LSD radix sort of the codes, 8 bits a pass; a pass whose digit is the same in every
//                     code is skipped on the device
//   k_oct_heads_*     the distinct codes: the occupied depth-16 cells in preorder
//   k_oct_nodes / k_oct_emit   the pruned tree, read off the sorted cells without building it (below)
//
// The tree is implicit in the sorted, distinct codes c[0..n).  The node of depth d above cell i is the run of codes with c >> 3(16-d)
// in common; it is FULL iff the run has 8^(16-d) codes, and because the codes are distinct and sorted that is
// c[s + 8^(16-d) - 1] == c[s] + 8^(16-d) - 1 at the run's aligned start s: one load.  After toMaxLikelihood every leaf has the same value, so
// prune() makes a node of depth >= 1 a leaf iff it is full, and a node is in the file iff no proper ancestor is full.  Element i
// starts the runs of depths D(i) .. 16, D(i) from the highest bit in which c[i] differs from c[i-1]; of those, depths F(i) .. 16
// are full (fullness is inherited downwards).  So element i owns the inner nodes of depths D(i) .. F(i)-1 - consecutive in preorder,
// an ancestor before its first descendant - and, unless an earlier element's full run covers it, the one leaf of depth F(i).
// Preorder positions are prefix sums of these counts over i; the two bytes of an inner node come from the eight child boundaries,
// found by bisection inside the node's run.  Sixteen levels are never materialised: the scratch is the sort's two buffers.
//
// Ordered compaction and the sort's core are orbx_cloud_dev.h's, here over the flat [B * cap] map: one-dimensional grids, k_oct_scan
// the scan of a count array.  The sort is of the bare 64-bit codes; its histogram is digit-major, [256][workgroups], and scanned by one
// workgroup per digit (k_oct_hscan), since a map has thousands of workgroups where a keyframe has tens; the passes that run are the
// digits in which two codes differ (codeOr ^ codeAnd).  The sizes live in a device record (OctState), launches are sized for the
// worst case and return early; the host reads nothing between the kernels.
#include "orbx_cloud_dev.h"
#include <math.h>
#include <algorithm>

#define OCT_MAX_POINTS (1 << 27)   // B * cap: 15 n + 1 inner nodes stay below 2^31
#define OCT_HEADER_MAX 192

struct OctXform { float m[12]; };   // rows 0..2 of M, row-major

struct OctState {
    unsigned long long codeOr, codeAnd;   // OR / AND of every valid point's code: the bits in which two codes differ are codeOr ^ codeAnd
    int32_t nIn, nValid, nCells, nInner, nLeaves, pad;
};

// bit p of x -> bit 3p (16 bits in, 46 bits out), and back
__device__ __forceinline__ unsigned long long oct_spread(unsigned long long x) {
    x &= 0xffffull;
    x = (x | (x << 32)) & 0x001f00000000ffffull;
    x = (x | (x << 16)) & 0x001f0000ff0000ffull;
    x = (x | (x << 8)) & 0x100f00f00f00f00full;
    x = (x | (x << 4)) & 0x10c30c30c30c30c3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}
__device__ __forceinline__ uint32_t oct_compact(unsigned long long x) {
    x &= 0x1249249249249249ull;
    x = (x ^ (x >> 2)) & 0x10c30c30c30c30c3ull;
    x = (x ^ (x >> 4)) & 0x100f00f00f00f00full;
    x = (x ^ (x >> 8)) & 0x001f0000ff0000ffull;
    x = (x ^ (x >> 16)) & 0x001f00000000ffffull;
    x = (x ^ (x >> 32)) & 0xffffull;
    return (uint32_t)x;
}

// OcTreeBaseImpl::coordToKeyChecked of one axis: (int)floor(resolution_factor * coordinate) + tree_max_val, valid in [0, 65535]
__device__ __forceinline__ bool oct_axis_key(float c, double resFactor, uint32_t &key) {
    const double t = floor(resFactor * (double)c);
    if (!(t >= -32768.0 && t <= 32767.0)) return false;   // (NaN and the infinities fail both)
    key = (uint32_t)((int)t + 32768);
    return true;
}

// element e of the flat [B * cap] map -> its code; false: outside its segment's count, not finite, or outside the tree
__device__ __forceinline__ bool oct_point_code(const orbx_cloud_point_t *__restrict__ pts, const int32_t *__restrict__ counts, int cap,
                                               int ntot, int e, const OctXform &M, double resFactor, unsigned long long &code) {
    if (e >= ntot) return false;
    const int b = e / cap;
    if (e - b * cap >= frame_points(counts, b, cap)) return false;
    const orbx_cloud_point_t p = pts[e];
    if (!(finite_bits(p.x) && finite_bits(p.y) && finite_bits(p.z))) return false;   // pcl::transformPointCloud skips it (the cloud is not dense)
    const float x = M.m[0] * p.x + M.m[1] * p.y + M.m[2] * p.z + M.m[3];
    const float y = M.m[4] * p.x + M.m[5] * p.y + M.m[6] * p.z + M.m[7];
    const float z = M.m[8] * p.x + M.m[9] * p.y + M.m[10] * p.z + M.m[11];
    uint32_t kx, ky, kz;
    if (!oct_axis_key(x, resFactor, kx) || !oct_axis_key(y, resFactor, ky) || !oct_axis_key(z, resFactor, kz)) return false;
    code = oct_spread(kx) | (oct_spread(ky) << 1) | (oct_spread(kz) << 2);
    return true;
}

// the record of a new call; nIn: the points of every segment
__global__ __launch_bounds__(CL_THREADS) void k_oct_init(OctState *__restrict__ st, const int32_t *__restrict__ counts, int B, int cap) {
    __shared__ int lds[4];
    int v = 0;
    for (int b = threadIdx.x; b < B; b += CL_THREADS) v += frame_points(counts, b, cap);
    int total;
    block_excl_scan(v, lds, total);
    if (threadIdx.x == 0) {
        st->codeOr = 0ull; st->codeAnd = ~0ull;
        st->nIn = total; st->nValid = st->nCells = st->nInner = st->nLeaves = st->pad = 0;
    }
}

__global__ __launch_bounds__(CL_THREADS) void k_oct_keys_count(const orbx_cloud_point_t *__restrict__ pts, const int32_t *__restrict__ counts,
                                                              int cap, int ntot, OctXform M, double resFactor, int32_t *__restrict__ blk) {
    __shared__ int segs[CL_SEGS];
    const int base = blockIdx.x * CL_TILE;
    bool flag[CL_ITERS];
    int rank[CL_ITERS];
#pragma unroll
    for (int k = 0; k < CL_ITERS; k++) {
        unsigned long long code;
        flag[k] = oct_point_code(pts, counts, cap, ntot, tile_elem(base, k), M, resFactor, code);
    }
    const int total = block_ranks(flag, rank, segs);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

// Per-workgroup counts -> exclusive offsets in place, the total to *tot.  One workgroup per array (blockIdx.x: array a of nblk counts,
// total tot[a]).  nElems (may be NULL): only the workgroups of the first *nElems elements have written a count.
__global__ __launch_bounds__(CL_THREADS) void k_oct_scan(int32_t *__restrict__ blk, int nblk, const int32_t *__restrict__ nElems,
                                                        int32_t *__restrict__ tot) {
    __shared__ int lds[4];
    const int nact = nElems ? min(nblk, (*nElems + CL_TILE - 1) / CL_TILE) : nblk;
    const int total = scan_counts(blk + (size_t)blockIdx.x * nblk, nact, lds);
    if (threadIdx.x == 0) tot[blockIdx.x] = total;
}

__global__ __launch_bounds__(CL_THREADS) void k_oct_keys_write(const orbx_cloud_point_t *__restrict__ pts, const int32_t *__restrict__ counts,
                                                              int cap, int ntot, OctXform M, double resFactor,
                                                              const int32_t *__restrict__ blk, unsigned long long *__restrict__ codes,
                                                              OctState *__restrict__ st) {
    __shared__ int segs[CL_SEGS];
    __shared__ unsigned long long red[4][2];
    const int base = blockIdx.x * CL_TILE;
    bool flag[CL_ITERS];
    int rank[CL_ITERS];
    unsigned long long code[CL_ITERS], vor = 0ull, vand = ~0ull;
#pragma unroll
    for (int k = 0; k < CL_ITERS; k++) {
        code[k] = 0ull;
        flag[k] = oct_point_code(pts, counts, cap, ntot, tile_elem(base, k), M, resFactor, code[k]);
        if (flag[k]) { vor |= code[k]; vand &= code[k]; }
    }
    const int total = block_ranks(flag, rank, segs);
    if (total == 0) return;   // (uniform over the workgroup)
    const int off = blk[blockIdx.x];
#pragma unroll
    for (int k = 0; k < CL_ITERS; k++)
        if (flag[k] && off + rank[k] < ntot) codes[off + rank[k]] = code[k];   // (always below ntot: kept as the store's bound)
    vor = wave_reduce(vor, [](unsigned long long x, unsigned long long y) { return x | y; });
    vand = wave_reduce(vand, [](unsigned long long x, unsigned long long y) { return x & y; });
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = vor; red[threadIdx.x >> 6][1] = vand; }
    __syncthreads();
    // OR / AND do not depend on the order; a workgroup whose bits the words hold already sends nothing (a stale read costs an atomic more)
    if (threadIdx.x == 0) {
        vor = red[0][0] | red[1][0] | red[2][0] | red[3][0];
        const unsigned long long cur = __hip_atomic_load(&st->codeOr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((cur | vor) != cur) atomicOr(&st->codeOr, vor);
    } else if (threadIdx.x == 64) {
        vand = red[0][1] & red[1][1] & red[2][1] & red[3][1];
        const unsigned long long cur = __hip_atomic_load(&st->codeAnd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((cur & vand) != cur) atomicAnd(&st->codeAnd, vand);
    }
}

// ---- the sort of the codes: six passes of 8 bits over the 48; pass p runs iff two codes differ in its digit, reads buffer
// oct_src(p) and writes the other, so the sorted codes end in buffer oct_src(6)
__device__ __forceinline__ bool oct_pass_runs(const OctState *st, int pass) {
    return (((st->codeOr ^ st->codeAnd) >> (8 * pass)) & 255ull) != 0ull;
}
__device__ __forceinline__ int oct_src(const OctState *st, int pass) {
    const unsigned long long v = st->codeOr ^ st->codeAnd;
    int r = 0;
    for (int q = 0; q < pass; q++) r ^= ((v >> (8 * q)) & 255ull) ? 1 : 0;
    return r;
}

// hist [256][nblk]: digit-major, so that k_oct_hscan's workgroup of a digit reads a contiguous row
__global__ __launch_bounds__(CL_THREADS) void k_oct_hist(int pass, const unsigned long long *__restrict__ codes2, int ntot,
                                                        const OctState *__restrict__ st, uint32_t *__restrict__ hist, int nblk) {
    __shared__ uint32_t h[256];
    const int base = blockIdx.x * CL_TILE, n = st->nValid;
    if (base >= n || !oct_pass_runs(st, pass)) return;
    const unsigned long long *codes = codes2 + (size_t)oct_src(st, pass) * ntot;
    radix_tile_hist(codes, n, base, pass, h);
    hist[(size_t)threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x];
}

// workgroup d: the running count of digit d over the workgroups in place, its total to digitTot[d]
__global__ __launch_bounds__(CL_THREADS) void k_oct_hscan(int pass, const OctState *__restrict__ st, uint32_t *__restrict__ hist, int nblk,
                                                         uint32_t *__restrict__ digitTot) {
    __shared__ int lds[4];
    const int n = st->nValid;
    if (n <= 0 || !oct_pass_runs(st, pass)) return;
    const int nact = min(nblk, (n + CL_TILE - 1) / CL_TILE);
    const int total = scan_counts((int32_t *)hist + (size_t)blockIdx.x * nblk, nact, lds);   // (counts of at most 2^27 codes)
    if (threadIdx.x == 0) digitTot[blockIdx.x] = (uint32_t)total;
}

__global__ __launch_bounds__(CL_THREADS) void k_oct_scatter(int pass, unsigned long long *__restrict__ codes2, int ntot,
                                                           const OctState *__restrict__ st, const uint32_t *__restrict__ hist, int nblk,
                                                           const uint32_t *__restrict__ digitTot) {
    __shared__ uint32_t seg[CL_SEGS][256];   // [segment][digit]: count, then first position
    __shared__ int lds[4];
    const int base = blockIdx.x * CL_TILE, n = st->nValid;
    if (base >= n || !oct_pass_runs(st, pass)) return;
    const int sb = oct_src(st, pass);
    const unsigned long long *src = codes2 + (size_t)sb * ntot;
    unsigned long long *dst = codes2 + (size_t)(sb ^ 1) * ntot;
    for (int s = 0; s < CL_SEGS; s++) seg[s][threadIdx.x] = 0u;
    int total;
    const uint32_t digitBase = (uint32_t)block_excl_scan((int)digitTot[threadIdx.x], lds, total);   // (its barriers also publish the zeros)
    unsigned long long key[CL_ITERS];
    bool flag[CL_ITERS];
#pragma unroll
    for (int k = 0; k < CL_ITERS; k++) {
        const int i = tile_elem(base, k);
        flag[k] = i < n;
        key[k] = flag[k] ? src[i] : 0ull;
    }
    radix_tile_scatter(
        key, flag, pass, n, seg, [&] { return digitBase + hist[(size_t)threadIdx.x * nblk + blockIdx.x]; },
        [&](int k, uint32_t o) { dst[o] = key[k]; });
}

// ---- the distinct codes

template <bool WRITE>
__global__ __launch_bounds__(CL_THREADS) void k_oct_heads(unsigned long long *__restrict__ codes2, int ntot, const OctState *__restrict__ st,
                                                         int32_t *__restrict__ blk) {
    __shared__ int segs[CL_SEGS];
    const int base = blockIdx.x * CL_TILE, n = st->nValid;
    if (base >= n) return;
    const int sb = oct_src(st, 6);
    const unsigned long long *codes = codes2 + (size_t)sb * ntot;
    bool flag[CL_ITERS];
    int rank[CL_ITERS];
    run_heads(codes, n, base, flag);
    const int total = block_ranks(flag, rank, segs);
    if (!WRITE) {
        if (threadIdx.x == 0) blk[blockIdx.x] = total;
        return;
    }
    unsigned long long *out = codes2 + (size_t)(sb ^ 1) * ntot;
    const int off = blk[blockIdx.x];
#pragma unroll
    for (int k = 0; k < CL_ITERS; k++)
        if (flag[k] && off + rank[k] < n) out[off + rank[k]] = codes[tile_elem(base, k)];   // (always below n: kept as the store's bound)
}

// ---- the pruned tree, read off the distinct sorted codes c[0..n)

// Element i: D = the shallowest depth at which it starts a run, F = the shallowest depth >= max(D, 1) at which its run is full,
// leaf = no earlier element's full run covers it.  It owns the inner nodes of depths D .. F-1 and, if leaf, the leaf of depth F.
__device__ __forceinline__ void oct_element(const unsigned long long *__restrict__ c, int n, int i, int &D, int &F, bool &leaf) {
    const unsigned long long ci = c[i];
    D = i == 0 ? 0 : 16 - (63 - __clzll((long long)(ci ^ c[i - 1]))) / 3;
    F = 16;
    for (int d = 15; d >= max(D, 1); d--) {
        const unsigned long long s1 = (1ull << (3 * (16 - d))) - 1ull;   // the run's size - 1
        if ((ci & s1) != 0ull || (unsigned long long)i + s1 >= (unsigned long long)n || c[i + s1] != ci + s1) break;
        F = d;
    }
    leaf = true;
    if (D >= 2) {   // the node of depth D-1 above i starts before i; the root (D-1 = 0) is never pruned
        const unsigned long long s1 = (1ull << (3 * (17 - D))) - 1ull, off = ci & s1;
        if (off <= (unsigned long long)i) {
            const unsigned long long s = (unsigned long long)i - off;
            if (s + s1 < (unsigned long long)n && c[s] == ci - off && c[s + s1] == ci - off + s1) leaf = false;
        }
    }
}

// inner nodes and leaves per workgroup: blk[0][.] / blk[1][.]
__global__ __launch_bounds__(CL_THREADS) void k_oct_nodes(const unsigned long long *__restrict__ codes2, int ntot, const OctState *__restrict__ st,
                                                         int32_t *__restrict__ blk, int nblk) {
    __shared__ int lds[4];
    const int base = blockIdx.x * CL_TILE, n = st->nCells;
    if (base >= n) return;
    const unsigned long long *c = codes2 + (size_t)(oct_src(st, 6) ^ 1) * ntot;
    int v = 0;
#pragma unroll
    for (int k = 0; k < CL_ITERS; k++) {
        const int i = tile_elem(base, k);
        if (i < n) {
            int D, F; bool leaf;
            oct_element(c, n, i, D, F, leaf);
            v += (F - D) | ((leaf ? 1 : 0) << 16);   // (at most 4 x 16 inner nodes a lane: the two counts share a word)
        }
    }
    // sum over the workgroup: 1024 x 16 inner nodes at most, 1024 leaves
    int inner = v & 0xffff, leaves = v >> 16, t0, t1;
    block_excl_scan(inner, lds, t0);
    block_excl_scan(leaves, lds, t1);
    if (threadIdx.x == 0) { blk[blockIdx.x] = t0; blk[nblk + blockIdx.x] = t1; }
}

// the totals -> the caller's record (and the device record, for k_oct_emit)
__global__ void k_oct_info(OctState *__restrict__ st, const int32_t *__restrict__ tot, int64_t dataCap, int64_t leafCap, int wantLeaves,
                           orbx_octree_info_t *__restrict__ info) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const bool any = st->nCells > 0;
    st->nInner = any ? tot[0] : 0;
    st->nLeaves = any ? tot[1] : 0;
    orbx_octree_info_t r;
    r.points_in = st->nIn;
    r.points_dropped = st->nIn - st->nValid;
    r.cells = st->nCells;
    r.leaves = st->nLeaves;
    r.tree_size = (int64_t)st->nInner + st->nLeaves;
    r.data_bytes = 2 * (int64_t)st->nInner;
    r.overflow = (r.data_bytes > dataCap || (wantLeaves && r.leaves > leafCap)) ? 1 : 0;
    r.reserved = 0;
    *info = r;
}

#define OE_WINDOW 4096   // inner nodes of a workgroup handed out at a time (a workgroup of a surface has some 350)

// Leaves at offset + rank.  The inner nodes are dealt out anew: a lane owns up to 16 of them per cell (cell 0 the root's whole spine)
// and most lanes one or none, so the lanes post theirs - (cell, depth), at the node's preorder rank inside the workgroup - to a list
// in LDS and every lane then takes every 256th: a node is eight bisections of the node's run, whoever does them.
__global__ __launch_bounds__(CL_THREADS) void k_oct_emit(const unsigned long long *__restrict__ codes2, int ntot, const OctState *__restrict__ st,
                                                        const int32_t *__restrict__ blk, int nblk, uint8_t *__restrict__ data, int64_t dataCap,
                                                        orbx_octree_leaf_t *__restrict__ leaves, int64_t leafCap) {
    __shared__ int segs[CL_SEGS];
    __shared__ int lds[4];
    __shared__ uint16_t work[OE_WINDOW];   // cell in the tile << 4 | depth
    const int base = blockIdx.x * CL_TILE, n = st->nCells;
    if (base >= n) return;
    const unsigned long long *c = codes2 + (size_t)(oct_src(st, 6) ^ 1) * ntot;
    int D[CL_ITERS], F[CL_ITERS], lrank[CL_ITERS], ipos[CL_ITERS];
    bool leaf[CL_ITERS];
#pragma unroll
    for (int k = 0; k < CL_ITERS; k++) {
        const int i = tile_elem(base, k);
        D[k] = F[k] = 0; leaf[k] = false;
        if (i < n) oct_element(c, n, i, D[k], F[k], leaf[k]);
    }
    block_ranks(leaf, lrank, segs);
    int nodes = 0;   // the workgroup's inner nodes
#pragma unroll
    for (int k = 0; k < CL_ITERS; k++) {   // (iteration k's elements come before iteration k+1's)
        int total;
        ipos[k] = nodes + block_excl_scan(F[k] - D[k], lds, total);
        nodes += total;
    }
    const int loff = blk[nblk + blockIdx.x];
    if (leaves) {
#pragma unroll
        for (int k = 0; k < CL_ITERS; k++) {
            if (!leaf[k] || loff + lrank[k] >= leafCap) continue;
            const unsigned long long ci = c[tile_elem(base, k)];
            orbx_octree_leaf_t l;
            l.kx = (uint16_t)oct_compact(ci); l.ky = (uint16_t)oct_compact(ci >> 1); l.kz = (uint16_t)oct_compact(ci >> 2);
            l.depth = (uint16_t)F[k];
            leaves[loff + lrank[k]] = l;
        }
    }
    const int64_t ioff = blk[blockIdx.x];
    for (int w0 = 0; w0 < nodes; w0 += OE_WINDOW) {
#pragma unroll
        for (int k = 0; k < CL_ITERS; k++)
            for (int d = D[k]; d < F[k]; d++) {
                const int p = ipos[k] + d - D[k] - w0;
                if (p >= 0 && p < OE_WINDOW) work[p] = (uint16_t)((tile_elem(0, k) << 4) | d);
            }
        __syncthreads();
        const int cnt = min(nodes - w0, OE_WINDOW);
        for (int p = threadIdx.x; p < cnt; p += CL_THREADS) {
            const int64_t at = 2 * (ioff + w0 + p);
            if (at + 2 > dataCap) break;   // (positions only grow with p)
            const int i = base + (work[p] >> 4), d = work[p] & 15;
            const unsigned long long ci = c[i];
            // the node's run is c[i .. hi); child q starts at the first code >= ((P << 3) + q) << sh: eight bisections side by side
            const int sh = 3 * (15 - d);
            const unsigned long long P8 = (ci >> (sh + 3)) << 3, span = 8ull << sh;
            const int hi = (unsigned long long)(n - i) > span ? i + (int)span : n;
            int lo[9], len = hi - i;
            lo[0] = i;
#pragma unroll
            for (int q = 1; q <= 8; q++) lo[q] = i;
            while (len > 1) {
                const int half = len >> 1;
#pragma unroll
                for (int q = 1; q <= 8; q++)
                    if (c[lo[q] + half - 1] < ((P8 + q) << sh)) lo[q] += half;
                len -= half;
            }
#pragma unroll
            for (int q = 1; q <= 8; q++)
                if (c[lo[q]] < ((P8 + q) << sh)) lo[q] += 1;
            uint32_t bits = 0u;
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const unsigned long long m = (unsigned long long)(lo[q + 1] - lo[q]);
                const uint32_t s = m == 0ull ? 0u : (m == (1ull << sh) ? 2u : 3u);   // absent, occupied leaf (a full child), has children
                bits |= s << (2 * q);
            }
            data[at] = (uint8_t)(bits & 255u);
            data[at + 1] = (uint8_t)(bits >> 8);
        }
        __syncthreads();
    }
}

// ---- host side

// the reference's transform_trans * transform_rot_x * transform_rot_y (src/pointcloudmapping.cc:198-223):
//   trans = [0 1 0; 0 0 -1; -1 0 0], rot_x = [0 1 0; -1 0 0; 0 0 1], rot_y = [0 0 -1; 0 1 0; 1 0 0]
//   trans * rot_x = [-1 0 0; 0 0 -1; 0 -1 0];  (trans * rot_x) * rot_y = [0 0 1; -1 0 0; 0 -1 0]:  x' = z, y' = -x, z' = -y
static const float kAxisSwap[12] = {0.f, 0.f, 1.f, 0.f, -1.f, 0.f, 0.f, 0.f, 0.f, -1.f, 0.f, 0.f};

static bool res_ok(double res) { return res > 0.0 && res < (double)INFINITY; }

// through the counting of the nodes: *d_info is complete after this
static int launch_octree_build(orbx_cloudmapper *m, const orbx_cloud_point_t *d_points, const int32_t *d_counts, int B, int cap,
                               const float *M16f, double res, int64_t data_cap, int64_t leaf_cap, int want_leaves,
                               orbx_octree_info_t *d_info, hipStream_t st) {
    const int ntot = B * cap, nblk = (ntot + CL_TILE - 1) / CL_TILE;
    int rc = reserve(&m->d_octCodes, &m->octCodeBytes, sizeof(unsigned long long) * 2 * (size_t)ntot);
    if (!rc) rc = reserve(&m->d_octBlk, &m->octBlkBytes, sizeof(int32_t) * 2 * (size_t)nblk);
    if (!rc) rc = reserve(&m->d_octHist, &m->octHistBytes, sizeof(uint32_t) * 256 * ((size_t)nblk + 1));
    if (!rc) rc = reserve(&m->d_octState, &m->octStateBytes, sizeof(OctState) + 2 * sizeof(int32_t));
    if (rc) return rc;
    OctXform M;
    memcpy(M.m, M16f ? M16f : kAxisSwap, sizeof(M.m));
    const double resFactor = 1.0 / res;   // OcTreeBaseImpl::setResolution
    unsigned long long *codes = (unsigned long long *)m->d_octCodes;
    int32_t *blk = (int32_t *)m->d_octBlk;
    uint32_t *hist = (uint32_t *)m->d_octHist, *digitTot = hist + 256 * (size_t)nblk;
    OctState *state = (OctState *)m->d_octState;
    int32_t *tot = (int32_t *)(m->d_octState + sizeof(OctState));
    const dim3 grid(nblk), block(CL_THREADS);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_oct_init, dim3(1), block, 0, st, state, d_counts, B, cap);
    hipLaunchKernelGGL(k_oct_keys_count, grid, block, 0, st, d_points, d_counts, cap, ntot, M, resFactor, blk);
    hipLaunchKernelGGL(k_oct_scan, dim3(1), block, 0, st, blk, nblk, (const int32_t *)nullptr, &state->nValid);
    hipLaunchKernelGGL(k_oct_keys_write, grid, block, 0, st, d_points, d_counts, cap, ntot, M, resFactor, (const int32_t *)blk, codes, state);
    for (int p = 0; p < 6; p++) {
        hipLaunchKernelGGL(k_oct_hist, grid, block, 0, st, p, (const unsigned long long *)codes, ntot, (const OctState *)state, hist, nblk);
        hipLaunchKernelGGL(k_oct_hscan, dim3(256), block, 0, st, p, (const OctState *)state, hist, nblk, digitTot);
        hipLaunchKernelGGL(k_oct_scatter, grid, block, 0, st, p, codes, ntot, (const OctState *)state, (const uint32_t *)hist, nblk,
                           (const uint32_t *)digitTot);
    }
    hipLaunchKernelGGL(k_oct_heads<false>, grid, block, 0, st, codes, ntot, (const OctState *)state, blk);
    hipLaunchKernelGGL(k_oct_scan, dim3(1), block, 0, st, blk, nblk, (const int32_t *)&state->nValid, &state->nCells);
    hipLaunchKernelGGL(k_oct_heads<true>, grid, block, 0, st, codes, ntot, (const OctState *)state, blk);
    hipLaunchKernelGGL(k_oct_nodes, grid, block, 0, st, (const unsigned long long *)codes, ntot, (const OctState *)state, blk, nblk);
    hipLaunchKernelGGL(k_oct_scan, dim3(2), block, 0, st, blk, nblk, (const int32_t *)&state->nCells, tot);
    hipLaunchKernelGGL(k_oct_info, dim3(1), dim3(64), 0, st, state, (const int32_t *)tot, data_cap, leaf_cap, want_leaves, d_info);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

static int launch_octree_emit(orbx_cloudmapper *m, int B, int cap, uint8_t *d_data, int64_t data_cap, orbx_octree_leaf_t *d_leaves,
                              int64_t leaf_cap, hipStream_t st) {
    const int ntot = B * cap, nblk = (ntot + CL_TILE - 1) / CL_TILE;
    hipLaunchKernelGGL(k_oct_emit, dim3(nblk), dim3(CL_THREADS), 0, st, (const unsigned long long *)m->d_octCodes, ntot,
                       (const OctState *)m->d_octState, (const int32_t *)m->d_octBlk, nblk, d_data, data_cap, d_leaves, leaf_cap);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbx_octree_device(orbx_cloudmapper_t *m, const orbx_cloud_point_t *d_points, const int32_t *d_counts, int B, int cap,
                                  const float *M16f, double res, uint8_t *d_data, int64_t data_cap, orbx_octree_leaf_t *d_leaves,
                                  int64_t leaf_cap, orbx_octree_info_t *d_info, void *stream) {
    if (!m || !d_points || !d_counts || !d_info || B < 1 || B > 65535 || cap < 1 || (long long)B * cap > OCT_MAX_POINTS || !res_ok(res) ||
        data_cap < 0 || (!d_data && data_cap > 0) || leaf_cap < 0 || ((uintptr_t)d_points & 3) || ((uintptr_t)d_leaves & 1) ||
        ((uintptr_t)d_info & 7)) {
        orbx_set_error("orbx_octree_device: bad arguments (res > 0 and finite, B * cap <= 2^27, capacities >= 0, d_info != NULL)");
        return ORBX_ERR_ARG;
    }
    ORBX_HIP(hipSetDevice(m->device));
    hipStream_t st = (hipStream_t)stream;
    int rc = launch_octree_build(m, d_points, d_counts, B, cap, M16f, res, data_cap, leaf_cap, d_leaves ? 1 : 0, d_info, st);
    if (!rc) rc = launch_octree_emit(m, B, cap, d_data, data_cap, d_leaves, leaf_cap, st);
    return rc;
}

extern "C" size_t orbx_octomap_bytes_bound(int64_t n) {
    if (n < 0) return 0;
    return (size_t)OCT_HEADER_MAX + (n > 0 ? 2 * (15 * (size_t)n + 1) : 0);
}

// OcTree::writeBinary's header (AbstractOcTree::writeBinary + binaryFileHeader); res as operator<< prints a double: %g
static int bt_header(char *buf, size_t cap, long long size, double res) {
    return snprintf(buf, cap,
                    "# Octomap OcTree binary file\n# (feel free to add / change comments, but leave the first line as it is!)\n#\n"
                    "id OcTree\nsize %lld\nres %g\ndata\n", size, res);
}

extern "C" int orbx_octomap_bt(orbx_cloudmapper_t *m, const orbx_cloud_point_t *points, int n, const float *M16f, double res, uint8_t *out,
                               size_t out_cap, size_t *n_bytes, orbx_octree_info_t *info) {
    if (!m || n < 0 || n > OCT_MAX_POINTS || (n > 0 && !points) || !res_ok(res) || !n_bytes || (!out && out_cap > 0)) {
        orbx_set_error("orbx_octomap_bt: bad arguments (n >= 0, res > 0 and finite, n_bytes != NULL, out != NULL unless out_cap is 0)");
        return ORBX_ERR_ARG;
    }
    *n_bytes = 0;
    orbx_octree_info_t r;
    memset(&r, 0, sizeof(r));
    char head[OCT_HEADER_MAX];
    uint8_t *d_data = nullptr;
    hipStream_t st = nullptr;
    if (n > 0) {
        ORBX_HIP(hipSetDevice(m->device));
        st = m->stream;
        int rc = reserve(&m->d_raw, &m->rawBytes, sizeof(orbx_cloud_point_t) * (size_t)n);
        if (!rc) rc = reserve(&m->d_cnt, &m->cntBytes, sizeof(int32_t) * 2 + sizeof(orbx_octree_info_t));
        if (rc) return rc;
        int32_t *d_cnt = (int32_t *)m->d_cnt;
        orbx_octree_info_t *d_info = (orbx_octree_info_t *)(m->d_cnt + 8);
        ORBX_HIP(hipMemcpyAsync(m->d_raw, points, sizeof(orbx_cloud_point_t) * (size_t)n, hipMemcpyHostToDevice, st));
        ORBX_HIP(hipMemcpyAsync(d_cnt, &n, sizeof(int32_t), hipMemcpyHostToDevice, st));
        rc = launch_octree_build(m, (const orbx_cloud_point_t *)m->d_raw, d_cnt, 1, n, M16f, res, INT64_MAX, 0, 0, d_info, st);
        if (rc) return rc;
        ORBX_HIP(hipMemcpyAsync(&r, d_info, sizeof(r), hipMemcpyDeviceToHost, st));
        ORBX_HIP(hipStreamSynchronize(st));   // (also: n and the info record were read and written before this returns)
    }
    const int hl = bt_header(head, sizeof(head), (long long)r.tree_size, res);
    const size_t need = (size_t)hl + (size_t)r.data_bytes;
    *n_bytes = need;
    if (info) *info = r;
    if (need > out_cap) {
        orbx_set_error("orbx_octomap_bt: the file has %zu bytes, out_cap %zu", need, out_cap);
        if (info) info->overflow = 1;
        return ORBX_ERR_CAPACITY;
    }
    memcpy(out, head, (size_t)hl);
    if (r.data_bytes > 0) {
        int rc = reserve(&m->d_out, &m->outBytes, (size_t)r.data_bytes);
        if (rc) return rc;
        d_data = m->d_out;
        rc = launch_octree_emit(m, 1, n, d_data, r.data_bytes, nullptr, 0, st);
        if (rc) return rc;
        ORBX_HIP(hipMemcpyAsync(out + hl, d_data, (size_t)r.data_bytes, hipMemcpyDeviceToHost, st));
        ORBX_HIP(hipStreamSynchronize(st));
    }
    return ORBX_OK;
}
