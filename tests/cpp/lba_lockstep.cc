// lba_lockstep.cc — the text of the k_lba_* kernels AND of their driver lba_drive (orb_slam2v2-1_amd/csrc/orbx_lba.hip) compiled for
// the host, every workgroup ONE thread, the workgroups of a launch one after the other, for tests/test_lba_cpu.py: every sum then
// runs in ascending order, which is the order of tests/lba_ref.py, so the two must give the same bits.  That pins the kernels'
// arithmetic, the ownership of the sums and the schedule (the stop polls included) without a GPU; what it cannot show - the
// 256-thread summation order, the barriers, the device's sin / cos / sqrt - is tests/test_lba_gpu.py's.  The entry points'
// argument checks (lba_check) run on the problem read and on broken copies of it, so that a sanitizer build covers them.
// Build with -ffp-contract=off, as the library is.
//   lba_lockstep IN OUT
//       IN:  int32 K, P, E, stop_at | orbb_schedule_t | orbb_keyframe_t[K] | orbb_point_t[P] | orbb_observation_t[E]
//            stop_at: 0 = no stop function, k > 0 = it answers 1 from its k-th call on, -1 = it always answers 0
//       OUT: float Tcw[K][16] | float pts[P][3] | uint8 erase[E] | orbb_info_t | double kf_est[K][7] | double pt_est[P][3]
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
#define LBA_LDS_BYTES (14 * 14 * 36 * 8)
uint8_t lba_lds[LBA_LDS_BYTES];                  // k_lba_solve's dynamic LDS (extern __shared__)

#include "orbx_lba.hip"

struct Stop { int at, calls; };
static int stop_fn(void *u) {
    Stop *s = (Stop *)u;
    s->calls++;
    return s->at > 0 && s->calls >= s->at;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: lba_lockstep IN OUT\n"); return 2; }
    static_assert(LBA_LDS_BYTES == LBA_LDS_POSES * LBA_LDS_POSES * 36 * 8, "LDS stage");
    static_assert(sizeof(orbb_keyframe_t) == 88 && sizeof(orbb_point_t) == 12 && sizeof(orbb_observation_t) == 24 &&
                  sizeof(orbb_schedule_t) == 36 && sizeof(orbb_info_t) == 44, "record layouts");
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
    // the checks the entry points make before they touch a device: this problem passes, broken ones do not
    if (lba_check("lockstep", kfs.data(), K, pts.data(), P, obs.data(), E, &sc, To.data(), Po.data(), er.data()) != ORBX_OK) { fprintf(stderr, "%s\n", g_err); return 3; }
    if (E >= 2 && K >= 1 && P >= 1) {
        std::vector<orbb_observation_t> bad(obs.begin(), obs.begin() + E);
        int wrong = 0;
        bad[1].kf = bad[0].kf; bad[1].pt = bad[0].pt;                                                          // a pair twice
        wrong += lba_check("lockstep", kfs.data(), K, pts.data(), P, bad.data(), E, &sc, To.data(), Po.data(), er.data()) != ORBX_ERR_ARG;
        bad[1] = obs[1]; bad[0].pt = P;                                                                      // an index out of range
        wrong += lba_check("lockstep", kfs.data(), K, pts.data(), P, bad.data(), E, &sc, To.data(), Po.data(), er.data()) != ORBX_ERR_ARG;
        bad[0] = obs[0]; bad[E - 1].inv_sigma2 = -1.f;
        wrong += lba_check("lockstep", kfs.data(), K, pts.data(), P, bad.data(), E, &sc, To.data(), Po.data(), er.data()) != ORBX_ERR_ARG;
        bad[E - 1] = obs[E - 1]; bad[E - 1].u = NAN;
        wrong += lba_check("lockstep", kfs.data(), K, pts.data(), P, bad.data(), E, &sc, To.data(), Po.data(), er.data()) != ORBX_ERR_ARG;
        std::vector<orbb_keyframe_t> bk(kfs.begin(), kfs.begin() + K);
        bk[K - 1].Tcw[7] = NAN;
        wrong += lba_check("lockstep", bk.data(), K, pts.data(), P, obs.data(), E, &sc, To.data(), Po.data(), er.data()) != ORBX_ERR_ARG;
        orbb_schedule_t bs = sc;
        bs.rounds = 3;
        wrong += lba_check("lockstep", kfs.data(), K, pts.data(), P, obs.data(), E, &bs, To.data(), Po.data(), er.data()) != ORBX_ERR_ARG;
        wrong += lba_check("lockstep", kfs.data(), K, pts.data(), P, nullptr, E, &sc, To.data(), Po.data(), er.data()) != ORBX_ERR_ARG;
        wrong += lba_check("lockstep", kfs.data(), K, pts.data(), P, obs.data(), E, &sc, To.data(), Po.data(), nullptr) != ORBX_ERR_ARG;
        if (wrong) return 3;
    }
    const LbaLayout L = lba_layout(kfs.data(), K, P, E);
    std::vector<uint8_t> mem(L.total, 0xEE);       // what fresh scratch held must not matter
    LbaMem M;
    M.d = mem.data(); M.h = mem.data();
    lba_stage(M.h, L, kfs.data(), K, pts.data(), P, obs.data(), E);
    Stop st = {hdr[3], 0};
    orbb_info_t info;
    memset(&info, 0xEE, sizeof(info));
    if (lba_drive(M, L, K, P, E, sc, hdr[3] ? stop_fn : nullptr, &st, &info) != ORBX_OK) return 4;
    lba_results(M.h, L, K, P, E, To.data(), Po.data(), er.data(), ke.data(), pe.data());
    f = fopen(argv[2], "wb");
    if (!f) return 1;
    fwrite(To.data(), 64, K, f); fwrite(Po.data(), 12, P, f); fwrite(er.data(), 1, E, f); fwrite(&info, sizeof(info), 1, f);
    fwrite(ke.data(), 56, K, f); fwrite(pe.data(), 24, P, f);
    fclose(f);
    return 0;
}
