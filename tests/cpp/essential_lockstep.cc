// essential_lockstep.cc — the text of the k_eg_* kernels AND of their driver eg_drive and symbolic step eg_symbolic
// (orb_slam2v2-1_amd/csrc/orbx_essential.hip) compiled for the host, every workgroup ONE thread, the workgroups of a launch one after
// the other, for tests/test_essential_cpu.py: every sum then runs in ascending order, which is the order of tests/essential_ref.py,
// so the two must give the same bits.  That pins the kernels' arithmetic, the ownership of the sums, the symbolic factorisation and
// the Levenberg-Marquardt schedule without a GPU; what it cannot show - the 256-thread summation order, the barriers, the device's
// sin / cos / acos / log / exp - is tests/test_essential_gpu.py's.  The entry point's argument checks (eg_check) run on the
// problem read and on broken copies of it, so that a sanitizer build covers them.  Build with -ffp-contract=off, as the library is.
//   essential_lockstep IN OUT
//       IN:  int32 N, E, P, fix_scale, iterations | orbg_vertex_t[N] | orbg_edge_t[E] | orbg_point_t[P]
//       OUT: float Tcw[N][16] | float pts[P][3] | double est[N][8] | orbg_info_t
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "orbx.h"

#define ORBX_EG_HOST
#include "hip_lockstep.h"
static char g_err[256];
static void orbx_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

#include "orbx_essential.hip"

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: essential_lockstep IN OUT\n"); return 2; }
    static_assert(sizeof(orbg_sim3_t) == 64 && sizeof(orbg_vertex_t) == 136 && sizeof(orbg_edge_t) == 12 && sizeof(orbg_point_t) == 16 &&
                  sizeof(orbg_info_t) == 304, "record layouts");
    FILE *f = fopen(argv[1], "rb");
    int32_t hdr[5];
    if (!f || fread(hdr, 4, 5, f) != 5) return 1;
    const int N = hdr[0], E = hdr[1], P = hdr[2], fix = hdr[3], its = hdr[4];
    if (N < 0 || E < 0 || P < 0) return 1;
    std::vector<orbg_vertex_t> vtx((size_t)N + 1);
    std::vector<orbg_edge_t> edges((size_t)E + 1);
    std::vector<orbg_point_t> pts((size_t)P + 1);
    if ((N && fread(vtx.data(), sizeof(orbg_vertex_t), N, f) != (size_t)N) || (E && fread(edges.data(), sizeof(orbg_edge_t), E, f) != (size_t)E) ||
        (P && fread(pts.data(), sizeof(orbg_point_t), P, f) != (size_t)P)) return 1;
    fclose(f);
    std::vector<float> To((size_t)N * 16 + 1), Po((size_t)P * 3 + 1);
    std::vector<double> est((size_t)N * 8 + 1);
    // the checks the entry point makes before it touches a device: this problem passes, broken ones do not
    if (eg_check("lockstep", vtx.data(), N, edges.data(), E, pts.data(), P, its, To.data(), Po.data()) != ORBX_OK) { fprintf(stderr, "%s\n", g_err); return 3; }
    if (E >= 2 && N >= 2) {
        int wrong = 0;
        std::vector<orbg_edge_t> be(edges.begin(), edges.begin() + E);
        be[0].j = be[0].i;                                                                           // i == j
        wrong += eg_check("lockstep", vtx.data(), N, be.data(), E, pts.data(), P, its, To.data(), Po.data()) != ORBX_ERR_ARG;
        be[0] = edges[0]; be[E - 1].i = N;                                                           // an index out of range
        wrong += eg_check("lockstep", vtx.data(), N, be.data(), E, pts.data(), P, its, To.data(), Po.data()) != ORBX_ERR_ARG;
        be[E - 1] = edges[E - 1]; be[1].j = -1;
        wrong += eg_check("lockstep", vtx.data(), N, be.data(), E, pts.data(), P, its, To.data(), Po.data()) != ORBX_ERR_ARG;
        be[1] = edges[1]; be[1].kind = 2;
        wrong += eg_check("lockstep", vtx.data(), N, be.data(), E, pts.data(), P, its, To.data(), Po.data()) != ORBX_ERR_ARG;
        std::vector<orbg_vertex_t> bv(vtx.begin(), vtx.begin() + N);
        bv[N - 1].Scw.t[1] = NAN;                                                                    // a value that is not finite
        wrong += eg_check("lockstep", bv.data(), N, edges.data(), E, pts.data(), P, its, To.data(), Po.data()) != ORBX_ERR_ARG;
        bv[N - 1] = vtx[N - 1]; bv[0].Scw.s = 0.0;                                                   // s <= 0
        wrong += eg_check("lockstep", bv.data(), N, edges.data(), E, pts.data(), P, its, To.data(), Po.data()) != ORBX_ERR_ARG;
        bv[0] = vtx[0]; bv[1].has_nc = 1; bv[1].Snc.s = -1.0;
        wrong += eg_check("lockstep", bv.data(), N, edges.data(), E, pts.data(), P, its, To.data(), Po.data()) != ORBX_ERR_ARG;
        bv[1] = vtx[1]; bv[1].has_nc = 0; bv[1].Snc.s = -1.0;                                        // Snc is not read without has_nc
        wrong += eg_check("lockstep", bv.data(), N, edges.data(), E, pts.data(), P, its, To.data(), Po.data()) != ORBX_OK;
        if (P >= 1) {
            std::vector<orbg_point_t> bp(pts.begin(), pts.begin() + P);
            bp[P - 1].ref = N;
            wrong += eg_check("lockstep", vtx.data(), N, edges.data(), E, bp.data(), P, its, To.data(), Po.data()) != ORBX_ERR_ARG;
            bp[P - 1] = pts[P - 1]; bp[0].y = INFINITY;
            wrong += eg_check("lockstep", vtx.data(), N, edges.data(), E, bp.data(), P, its, To.data(), Po.data()) != ORBX_ERR_ARG;
            wrong += eg_check("lockstep", vtx.data(), N, edges.data(), E, pts.data(), P, its, To.data(), nullptr) != ORBX_ERR_ARG;
        }
        wrong += eg_check("lockstep", vtx.data(), N, edges.data(), E, pts.data(), P, ORBG_MAX_ITERATIONS + 1, To.data(), Po.data()) != ORBX_ERR_ARG;
        wrong += eg_check("lockstep", vtx.data(), N, nullptr, E, pts.data(), P, its, To.data(), Po.data()) != ORBX_ERR_ARG;
        wrong += eg_check("lockstep", vtx.data(), N, edges.data(), E, pts.data(), P, its, nullptr, Po.data()) != ORBX_ERR_ARG;
        if (wrong) return 3;
    }
    const EgSym S = eg_symbolic(vtx.data(), N, edges.data(), E);
    const EgLayout L = eg_layout(S, N, E, P);
    std::vector<uint8_t> mem(L.total, 0xEE);       // what fresh scratch held must not matter
    EgMem M;
    M.d = mem.data(); M.h = mem.data();
    eg_stage(M.h, L, S, vtx.data(), N, edges.data(), E, pts.data(), P);
    orbg_info_t info;
    memset(&info, 0xEE, sizeof(info));
    if (eg_drive(M, L, S, N, E, P, fix, its, &info) != ORBX_OK) return 4;
    eg_results(M.h, L, N, P, To.data(), Po.data(), est.data());
    f = fopen(argv[2], "wb");
    if (!f) return 1;
    fwrite(To.data(), 64, N, f); fwrite(Po.data(), 12, P, f); fwrite(est.data(), 64, N, f); fwrite(&info, sizeof(info), 1, f);
    fclose(f);
    return 0;
}
