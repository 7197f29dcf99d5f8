// div_rn_check.cc — orbx_div_rn (orb_slam2v2-1_amd/csrc/orbx_div_rn.h, the division of k_rect_map) against x86 division on the
// host: every pair of a grid of special operands (zeros, infinities, NaN, subnormals, extremes) and random operands whose quotients
// fall in the normal range, below it (subnormal and underflow to zero), above it (overflow) and on exactly representable values.
// Prints "<mismatches> <cases>"; exit status 1 on any mismatch.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include "orbx_div_rn.h"

static uint64_t bits(double d) { uint64_t u; std::memcpy(&u, &d, 8); return u; }
static double from(uint64_t u) { double d; std::memcpy(&d, &u, 8); return d; }

int main() {
    long bad = 0, n = 0;
    auto check = [&](double a, double b) {
        const double got = orbx_div_rn(a, b), want = a / b;
        n++;
        if ((std::isnan(got) && std::isnan(want)) || bits(got) == bits(want)) return;
        if (bad++ < 10) std::printf("mismatch %a / %a: %a, x86 %a\n", a, b, got, want);
    };
    const double sp[] = {0.0, -0.0, 1.0, -1.0, 3.0, 0.1, -7.5, INFINITY, -INFINITY, NAN, DBL_MAX, -DBL_MAX, DBL_MIN, -DBL_MIN,
                         from(1), from(2), from(3), from(0x000fffffffffffffull), from(0x0008000000000000ull), DBL_MIN * 1.5,
                         std::ldexp(1.0, -1000), std::ldexp(1.0, 1000), 1.0 - DBL_EPSILON / 2, 1.0 + DBL_EPSILON, 1e-310, 1e308};
    for (double a : sp)
        for (double b : sp) check(a, b);
    std::mt19937_64 g(12345);
    auto with_exp = [&](int e) { return from((g() & 0x800fffffffffffffull) | ((uint64_t)(e + 1023) << 52)); };
    for (long i = 0; i < 4000000; i++) {
        switch (i % 6) {
        case 0: check(from(g()), from(g())); break;                                    // any bit patterns
        case 1: check(with_exp((int)(g() % 60) - 30), with_exp((int)(g() % 60) - 30)); break;   // normal quotients
        case 2: check(with_exp(-1000 - (int)(g() % 22)), with_exp(20 + (int)(g() % 60))); break; // subnormal / zero quotients
        case 3: check(with_exp(990 + (int)(g() % 33)), with_exp(-40 - (int)(g() % 30))); break;  // near and past overflow
        case 4: {                                                                       // exact quotients: q * b rounds to a
            const double b = with_exp((int)(g() % 40) - 20), q = (double)(int64_t)(g() % 2000001 - 1000000) / 1024.0;
            check(q * b, b);
            break;
        }
        default: check(1.0, with_exp((int)(g() % 2046) - 1022)); break;               // reciprocals over the whole range
        }
    }
    std::printf("%ld %ld\n", bad, n);
    return bad != 0;
}
