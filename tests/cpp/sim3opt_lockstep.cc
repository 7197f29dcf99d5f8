// sim3opt_lockstep.cc — the text of k_sim3_opt (orb_slam2v2-1_amd/csrc/orbx_sim3opt.hip) compiled for the host and run as ONE thread,
// for tests/test_sim3opt_cpu.py: with one thread the kernel sums its matches in ascending order, which is the order of
// tests/sim3opt_ref.py, so the two must give the same bits.  That pins the kernel's arithmetic and control flow without a GPU; what
// it cannot show - the 256-thread summation order, the barriers, the device's exp / sin / cos - is tests/test_sim3opt_gpu.py's.
// The entry points' argument checks (s3o_check) are compiled too and run on the problem read, so that a sanitizer build of this
// program covers them.  Build with -ffp-contract=off, as the library is.
//   sim3opt_lockstep IN OUT
//       IN:  int32 n | orbz_sim3_problem_t | orbz_sim3_match_t[n]
//       OUT: float S12[16] | int32 ninliers | orbz_sim3_info_t | uint8 dropped[n]
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "orbx.h"

#define ORBX_SIM3OPT_HOST
#include "hip_lockstep.h"
static char g_err[256];
static void orbx_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
uint8_t s3o_lds[1024 * 48];                  // the kernel's dynamic LDS (extern __shared__)

#include "orbx_sim3opt.hip"

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: sim3opt_lockstep IN OUT\n"); return 2; }
    static_assert(sizeof(s3o_lds) == S3O_LDS_ROWS * sizeof(S3oRow), "LDS stage");
    static_assert(sizeof(orbz_sim3_match_t) == 48 && sizeof(orbz_sim3_problem_t) == 220 && sizeof(orbz_sim3_info_t) == 96, "record layouts");
    FILE *f = fopen(argv[1], "rb");
    int32_t n = 0;
    S3oProblem pr;
    if (!f || fread(&n, 4, 1, f) != 1 || n < 0 || fread(&pr.p, sizeof(pr.p), 1, f) != 1) return 1;
    pr.off = 0; pr.n = n;
    std::vector<orbz_sim3_match_t> m((size_t)n + 1);
    std::vector<S3oRow> rows((size_t)n + 1);
    std::vector<uint8_t> over((size_t)n + 1, 0xAB), dropped((size_t)n + 1, 0xCD);
    if (n && fread(m.data(), sizeof(orbz_sim3_match_t), n, f) != (size_t)n) return 1;
    fclose(f);
    float S[16];
    int32_t ninl = -1;
    orbz_sim3_info_t info;
    memset(&info, 0xEE, sizeof(info));
    // the checks the entry points make before they touch a device: this problem passes, four broken ones do not
    const int32_t off[2] = {0, n}, dec[3] = {0, 1, 0}, neg[2] = {-1, 0};
    if (s3o_check("lockstep", m.data(), off, 1, &pr.p, S, dropped.data(), &ninl) != ORBX_OK) { fprintf(stderr, "%s\n", g_err); return 3; }
    orbz_sim3_problem_t badp[2] = {pr.p, pr.p};
    badp[0].th2 = -1.f;
    orbz_sim3_match_t badm = {};
    badm.inv_sigma2_2 = NAN;
    if (s3o_check("lockstep", m.data(), nullptr, 1, &pr.p, S, dropped.data(), &ninl) != ORBX_ERR_ARG ||
        s3o_check("lockstep", m.data(), dec, 2, badp + 1, S, dropped.data(), &ninl) != ORBX_ERR_ARG ||
        s3o_check("lockstep", m.data(), neg, 1, &pr.p, S, dropped.data(), &ninl) != ORBX_ERR_ARG ||
        s3o_check("lockstep", m.data(), off, 1, badp, S, dropped.data(), &ninl) != ORBX_ERR_ARG ||
        s3o_check("lockstep", &badm, dec, 1, &pr.p, S, dropped.data(), &ninl) != ORBX_ERR_ARG ||
        s3o_check("lockstep", nullptr, dec, 1, &pr.p, S, dropped.data(), &ninl) != ORBX_ERR_ARG) return 3;
    k_sim3_opt(&pr, m.data(), rows.data(), over.data(), dropped.data(), S, &ninl, &info);
    f = fopen(argv[2], "wb");
    if (!f) return 1;
    fwrite(S, 64, 1, f); fwrite(&ninl, 4, 1, f); fwrite(&info, sizeof(info), 1, f); fwrite(dropped.data(), 1, n, f);
    fclose(f);
    return 0;
}
