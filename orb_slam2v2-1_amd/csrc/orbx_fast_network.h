// orbx_fast_network.h — the min/max network of the FAST-9/16 segment test, written once.
//
// For a ring p[0..15] (indices mod 16) the segment test of cv::FAST needs, over the sixteen nine-arcs a = {p[s], .., p[s+8]},
//     A = min over the arcs of (max of the arc)        and its dual        B = max over the arcs of (min of the arc).
// fast_arc_extreme computes ONE of them from two 3-input operations `in` (inside an arc) and `out` (across arcs): in = max and
// out = min give A, exchanged they give B.  A 2-input operation is the 3-input one with an operand repeated.  The network takes
// 29 operations per polarity (the pairing of neighbouring arcs over eight 4-windows it replaces took 36):
//   * the arcs are grouped by eight, starts i .. i+7 for i = 0 and 8.  All eight hold p[i+7] and p[i+8];
//   * the arcs i .. i+3 also share T = in(p[i+4..i+6]) and differ in a private part I0; the arcs i+4 .. i+7 share
//     Y = in(p[i+9..i+11]) and differ in I4.  T and Y are 3-windows that the OTHER half of the group needs inside its private
//     part, so each is computed once and used twice;
//   * the private parts of the arcs i .. i+3 are the 3-windows {i,i+1,i+2}, {i+1,i+2,i+9}, {i+2,i+9,i+10} and Y itself; the
//     first two share two elements, out(in(a,b,x), in(a,b,y)) = in(a, b, out(x,y)) (distributivity), so I0 is three terms under
//     one `out`.  I4 likewise from T, {i+5,i+6,i+13}, {i+6,i+13,i+14} and {i+13,i+14,i+15}.
// The expressions are lattice polynomials (min and max over a total order), and two lattice polynomials are equal on every input
// iff they are equal on every input from {0,1}: a value v enters only through comparisons, so thresholding all inputs at any
// level t commutes with min and max, and two polynomials that differed somewhere would differ at the threshold between their two
// results.  tests/test_fast_network_cpu.py runs all 65 536 such rings (and 10^6 random ones) against the sixteen-arc definition.
//
// Generic over the value type and the operations: the device instantiates it on packed f16 pairs with one pinned instruction per
// operation (orbx_fast.hip), the host check on plain integers.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ORBX_NET_FN __host__ __device__ __forceinline__
#else
#define ORBX_NET_FN inline
#endif

// in / out: callables (a, b, c) -> T.  14 operations per group of eight arcs, two groups, one to join them.
template <class T, class In, class Out>
ORBX_NET_FN T fast_arc_extreme(const T (&p)[16], In in, Out out) {
    T G[2];
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
    for (int h = 0; h < 2; h++) {
        const int i = 8 * h;
#define ORBX_NET_P(k) p[(i + (k)) & 15]
        const T Y = in(ORBX_NET_P(9), ORBX_NET_P(10), ORBX_NET_P(11));
        const T Tt = in(ORBX_NET_P(4), ORBX_NET_P(5), ORBX_NET_P(6));
        const T u = in(ORBX_NET_P(1), ORBX_NET_P(2), out(ORBX_NET_P(0), ORBX_NET_P(9), ORBX_NET_P(9)));
        const T I0 = out(u, in(ORBX_NET_P(2), ORBX_NET_P(9), ORBX_NET_P(10)), Y);          // arcs i .. i+3: their private part
        const T w = in(ORBX_NET_P(13), ORBX_NET_P(14), out(ORBX_NET_P(6), ORBX_NET_P(15), ORBX_NET_P(15)));
        const T I4 = out(Tt, in(ORBX_NET_P(5), ORBX_NET_P(6), ORBX_NET_P(13)), w);         // arcs i+4 .. i+7
        const T lo4 = in(Tt, ORBX_NET_P(3), I0), hi4 = in(Y, ORBX_NET_P(12), I4);
        G[h] = in(ORBX_NET_P(7), ORBX_NET_P(8), out(lo4, hi4, hi4));
#undef ORBX_NET_P
    }
    return out(G[0], G[1], G[1]);
}
