// Host check of csrc/orbx_fast_network.h (built and run by test_fast_network_cpu.py): the network on plain integers against the
// literal definition of the FAST-9/16 segment test - sixteen arcs of nine ring pixels, both polarities.
//   1. all 65 536 rings with values from {0,1}: the proof (see the header: lattice polynomials);
//   2. 10^6 random rings of values 0..255 from a fixed seed: the same on the values the kernels see.
// Prints one line per part and exits non-zero at the first mismatch.
#include <cstdint>
#include <cstdio>

#include "orbx_fast_network.h"

struct Min3 {
    int operator()(int a, int b, int c) const { const int m = a < b ? a : b; return m < c ? m : c; }
};
struct Max3 {
    int operator()(int a, int b, int c) const { const int m = a > b ? a : b; return m > c ? m : c; }
};

// A = min over the 16 nine-arcs of the arc's maximum, B = max over the arcs of the arc's minimum
static void literal(const int (&p)[16], int &A, int &B) {
    A = 1 << 30;
    B = -(1 << 30);
    for (int s = 0; s < 16; s++) {
        int mx = p[s], mn = p[s];
        for (int k = 1; k < 9; k++) {
            const int v = p[(s + k) & 15];
            if (v > mx) mx = v;
            if (v < mn) mn = v;
        }
        if (mx < A) A = mx;
        if (mn > B) B = mn;
    }
}

static bool check(const int (&p)[16], const char *what, unsigned long n) {
    int A, B;
    literal(p, A, B);
    const int a = fast_arc_extreme(p, Max3(), Min3()), b = fast_arc_extreme(p, Min3(), Max3());
    if (a == A && b == B) return true;
    std::printf("MISMATCH %s case %lu: ring", what, n);
    for (int k = 0; k < 16; k++) std::printf(" %d", p[k]);
    std::printf(" | A %d (literal %d) B %d (literal %d)\n", a, A, b, B);
    return false;
}

int main() {
    int p[16];
    for (unsigned long m = 0; m < 65536ul; m++) {
        for (int k = 0; k < 16; k++) p[k] = (int)((m >> k) & 1ul);
        if (!check(p, "binary", m)) return 1;
    }
    std::printf("binary rings: 65536 ok\n");
    uint64_t s = 0x9E3779B97F4A7C15ull;   // xorshift64*, fixed seed
    for (unsigned long n = 0; n < 1000000ul; n++) {
        for (int k = 0; k < 16; k++) {
            s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
            p[k] = (int)(((s * 0x2545F4914F6CDD1Dull) >> 56) & 255u);
        }
        if (!check(p, "random", n)) return 1;
    }
    std::printf("random rings: 1000000 ok\n");
    return 0;
}
