// orbx_div_rn.h — correctly rounded double division without fused multiply-adds (k_rect_map, orbx_rectify.hip).
// Host and device code: the host build is what tests/test_div_rn_cpu.py checks against x86 division.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define ORBX_HD __host__ __device__
#else
#define ORBX_HD
#endif

// The hardware sequence for `/` refines a reciprocal estimate with v_fma_f64; the map must not contain one,
// so the quotient of the significands is formed by restoring long division in integers and rounded to nearest even: the IEEE result,
// as x86's divsd gives it, for every input (zeros, infinities, NaN, subnormal operands and results).
ORBX_HD static inline double orbx_div_rn(double a, double b) {
    uint64_t ua, ub;
    memcpy(&ua, &a, 8); memcpy(&ub, &b, 8);
    const uint64_t sign = (ua ^ ub) & 0x8000000000000000ull, frac = (1ull << 52) - 1;
    int ea = (int)((ua >> 52) & 0x7ff), eb = (int)((ub >> 52) & 0x7ff);
    uint64_t ma = ua & frac, mb = ub & frac, out;
    if ((ea == 0x7ff && ma) || (eb == 0x7ff && mb)) return a + b;   // a NaN operand: a NaN
    const uint64_t inf = 0x7ff0000000000000ull, nan = 0x7ff8000000000000ull;
    if (ea == 0x7ff) out = eb == 0x7ff ? nan : sign | inf;
    else if (eb == 0x7ff) out = sign;
    else if (ea == 0 && ma == 0) out = (eb == 0 && mb == 0) ? nan : sign;
    else if (eb == 0 && mb == 0) out = sign | inf;
    else {
        // a = ma * 2^(ea - 1075), ma in [2^52, 2^53) (subnormals normalised)
        if (ea) ma |= 1ull << 52; else { ea = 1; while (!(ma >> 52)) { ma <<= 1; ea--; } }
        if (eb) mb |= 1ull << 52; else { eb = 1; while (!(mb >> 52)) { mb <<= 1; eb--; } }
        if (ma < mb) { ma <<= 1; ea--; }   // ma / mb in [1, 2)
        uint64_t q = 0, r = ma;
        for (int i = 0; i < 55; i++) {      // q = floor(ma / mb * 2^54), 55 bits
            q <<= 1;
            if (r >= mb) { r -= mb; q |= 1; }
            r <<= 1;
        }
        int be = ea - eb + 1023;            // biased exponent of the result's leading bit
        int drop = 2;
        if (be < 1) { drop += 1 - be; be = 1; }   // subnormal result: fewer significand bits
        if (drop > 60) out = sign;
        else {
            uint64_t m = q >> drop;
            const uint64_t rem = q & ((1ull << drop) - 1), half = 1ull << (drop - 1);
            if (rem > half || (rem == half && (r != 0 || (m & 1)))) m++;
            if ((uint64_t)(be - 1) + (m >> 52) >= 0x7ff) out = sign | inf;
            else out = sign | (((uint64_t)(be - 1) << 52) + m);   // (m = 2^53 after rounding carries into the exponent)
        }
    }
    double d;
    memcpy(&d, &out, 8);
    return d;
}
