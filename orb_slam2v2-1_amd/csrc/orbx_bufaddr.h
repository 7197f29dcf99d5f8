// Buffer-descriptor addressing: address = wave-uniform base (128-bit descriptor in SGPRs) + the lane's 32-bit byte offset (voffset)
// + a scalar byte offset such as the row (soffset).  A plain pointer `base + row + lane` costs a 64-bit vector add per access
// (the compiler reassociates the scalar row onto the vector unit); a buffer access costs no vector instruction at all.
//
// Rules:
//  * ONE descriptor per (image, buffer), built only from kernel arguments, blockIdx-derived values and readfirstlane'd values:
//    a descriptor the compiler cannot prove wave-uniform is wrapped in a serialising loop around every access.
//  * `bytes` must cover every byte the accesses touch, counted from `base`: a load past the range returns 0 SILENTLY and a store
//    past it is dropped (no fault), so a short range corrupts results instead of crashing.  The ranges used here hold for the
//    SUM of the lane offset, the scalar offset and the access size, so they do not depend on which part the hardware checks.
//  * offsets are unsigned 32-bit byte counts: the buffer (a padded pyramid level, a level's slot block) is far smaller than 4 GiB.
#pragma once
#include <stdint.h>

typedef __amdgpu_buffer_rsrc_t orbx_buf_t;
typedef uint32_t orbx_u32x2 __attribute__((ext_vector_type(2)));

// raw buffer (stride 0, no swizzle), 32-bit data format word of gfx9: offsets are plain byte offsets
__device__ __forceinline__ orbx_buf_t buf_make(const void *base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), (short)0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ uint2 buf_load_b64(orbx_buf_t r, uint32_t voff, uint32_t soff) {
    const orbx_u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, (int)soff, 0);
    return make_uint2(v.x, v.y);
}
__device__ __forceinline__ void buf_store_b16(orbx_buf_t r, uint32_t voff, uint32_t soff, uint16_t v) {
    __builtin_amdgcn_raw_buffer_store_b16(v, r, (int)voff, (int)soff, 0);
}
__device__ __forceinline__ void buf_store_b32(orbx_buf_t r, uint32_t voff, uint32_t soff, uint32_t v) {
    __builtin_amdgcn_raw_buffer_store_b32(v, r, (int)voff, (int)soff, 0);
}
