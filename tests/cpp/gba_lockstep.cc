// gba_lockstep.cc — lba_lockstep.cc's program on the BLOCKED reduced-system path (k_gba_schur, k_gba_diag / rows / trail, the blocked
// substitutions; orb_slam2v2-1_amd/csrc/orbx_lba.hip) for tests/test_gba_cpu.py: the kernels' text and lba_drive(blocked = 1) compiled
// for the host, every workgroup ONE thread, the workgroups of a launch one after the other.  The blocked factorisation gives every
// entry the operations of the one-workgroup one in the same order, so the outputs must equal tests/lba_ref.py's byte for byte; what
// the program cannot show - the 256-thread sums, the barriers, the tiles running side by side - is tests/test_gba_gpu.py's.
// Build with -ffp-contract=off, as the library is.
//   gba_lockstep IN OUT
//       IN:  int32 K, P, E, stop_at | orbb_schedule_t | orbb_keyframe_t[K] | orbb_point_t[P] | orbb_observation_t[E]
//            stop_at: 0 = no stop function, k > 0 = it answers 1 from its k-th call on, -1 = it always answers 0
//       OUT: float Tcw[K][16] | float pts[P][3] | uint8 erase[E] | orbb_info_t | double kf_est[K][7] | double pt_est[P][3] |
//            orbb_blocked_info_t
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "orbx.h"

#define ORBX_LBA_HOST
#include "hip_lockstep.h"
static char g_err[256];
static void orbx_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
uint8_t lba_lds[8];                              // k_lba_solve's dynamic LDS: the blocked path never launches it

#include "orbx_lba.hip"

struct Stop { int at, calls; };
static int stop_fn(void *u) {
    Stop *s = (Stop *)u;
    s->calls++;
    return s->at > 0 && s->calls >= s->at;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: gba_lockstep IN OUT\n"); return 2; }
    static_assert(sizeof(orbb_blocked_info_t) == 40 && sizeof(orbb_info_t) == 44 && sizeof(orbb_schedule_t) == 36, "record layouts");
    FILE *f = fopen(argv[1], "rb");
    int32_t hdr[4];
    orbb_schedule_t sc;
    if (!f || fread(hdr, 4, 4, f) != 4 || fread(&sc, sizeof(sc), 1, f) != 1) return 1;
    const int K = hdr[0], P = hdr[1], E = hdr[2];
    if (K < 0 || P < 0 || E < 0) return 1;
    std::vector<orbb_keyframe_t> kfs((size_t)K + 1);
    std::vector<orbb_point_t> pts((size_t)P + 1);
    std::vector<orbb_observation_t> obs((size_t)E + 1);
    if ((K && fread(kfs.data(), sizeof(orbb_keyframe_t), K, f) != (size_t)K) || (P && fread(pts.data(), sizeof(orbb_point_t), P, f) != (size_t)P) ||
        (E && fread(obs.data(), sizeof(orbb_observation_t), E, f) != (size_t)E)) return 1;
    fclose(f);
    std::vector<float> To((size_t)K * 16 + 1), Po((size_t)P * 3 + 1);
    std::vector<uint8_t> er((size_t)E + 1, 0xCD);
    std::vector<double> ke((size_t)K * 7 + 1), pe((size_t)P * 3 + 1);
    if (lba_check("lockstep", kfs.data(), K, pts.data(), P, obs.data(), E, &sc, To.data(), Po.data(), er.data()) != ORBX_OK) { fprintf(stderr, "%s\n", g_err); return 3; }
    const LbaLayout L = lba_layout(kfs.data(), K, P, E, obs.data(), 1);
    std::vector<uint8_t> mem(L.total, 0xEE);       // what fresh scratch held must not matter: S is cleared before every trial
    LbaMem M;
    M.d = mem.data(); M.h = mem.data();
    lba_stage(M.h, L, kfs.data(), K, pts.data(), P, obs.data(), E);
    Stop st = {hdr[3], 0};
    orbb_info_t info;
    orbb_blocked_info_t binfo;
    memset(&info, 0xEE, sizeof(info));
    memset(&binfo, 0xEE, sizeof(binfo));
    if (lba_drive(M, L, K, P, E, sc, hdr[3] ? stop_fn : nullptr, &st, &info, 1, &binfo) != ORBX_OK) return 4;
    lba_results(M.h, L, K, P, E, To.data(), Po.data(), er.data(), ke.data(), pe.data());
    f = fopen(argv[2], "wb");
    if (!f) return 1;
    fwrite(To.data(), 64, K, f); fwrite(Po.data(), 12, P, f); fwrite(er.data(), 1, E, f); fwrite(&info, sizeof(info), 1, f);
    fwrite(ke.data(), 56, K, f); fwrite(pe.data(), 24, P, f); fwrite(&binfo, sizeof(binfo), 1, f);
    fclose(f);
    return 0;
}
