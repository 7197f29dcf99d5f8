// hip_lockstep.h — the HIP keywords and built-ins the solver kernels use, for a grid run as ONE thread per workgroup, the workgroups
// one after the other: what the *_lockstep.cc programs include before a kernel's text.  The program sets blockIdx.x itself.
#pragma once
#include <stdint.h>
#include <string.h>
#define __global__
#define __device__
#define __forceinline__ inline
#define __shared__
#define __launch_bounds__(x)
#define __restrict__
#define __align__(x)
struct Idx3 { int x; };
static const Idx3 threadIdx = {0}, gridDim = {1};
static Idx3 blockIdx = {0};
static inline void __syncthreads() {}
static inline int atomicAdd(int *p, int v) { const int old = *p; *p += v; return old; }
static inline unsigned long long __ballot(int p) { return p ? 1ull : 0ull; }
static inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
static inline double __shfl_xor(double v, int, int) { return v; }   // never reached: a wave of one lane has no butterfly steps
static inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float __uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
