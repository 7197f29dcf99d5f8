// pnp_lockstep.cc — the text of k_pnp_ransac / k_pnp_refine / k_pnp_select (orb_slam2v2-1_amd/csrc/orbx_pnp.hip) compiled for the
// host and run as ONE thread per workgroup, the workgroups one after the other, for tests/test_pnp_cpu.py: every output byte must
// equal tests/pnp_ref.py's.  That pins the kernels' arithmetic and control flow without a GPU; what it cannot show - the sharing of
// entries and points among lanes, the barriers, the ballots, the device's double division and square root - is
// tests/test_pnp_gpu.py's.  Build with -ffp-contract=off, as the library is.
//   pnp_lockstep IN OUT
//       IN:  int32 B | int32 offsets[B+1] | int32 set_offsets[B+1] | orbp_problem_t problems[B] | orbp_corr_t corrs[offsets[B]] |
//            int32 sets[set_offsets[B]][4] | uint8 prior_best_flags[offsets[B]]
//       OUT: orbp_pnp_info_t infos[B] | int32 counts[nh] | int32 choices[nh] | int32 refined_counts[nh + B] | uint8 inliers[np] |
//            uint8 best_flags[np] | double models[nh][12] | float tcws[nh][16] | double refined_models[nh + B][12] |
//            float refined_tcws[nh + B][16] | uint8 flags[sum its x n] | uint8 refined_flags[sum (its + 1) x n]
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "orbx.h"

#define ORBX_PNP_HOST
#include "hip_lockstep.h"

#include "orbx_pnp.hip"

template <typename T> static bool rd(FILE *f, std::vector<T> &v, size_t n) { v.assign(n + 1, T()); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: pnp_lockstep IN OUT\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    int32_t B;
    if (!f || fread(&B, 4, 1, f) != 1 || B < 1 || B > 1024) return 1;
    std::vector<int32_t> off, soff, sets, hprob, rprob;
    std::vector<orbp_problem_t> prob;
    std::vector<orbp_corr_t> corrs;
    std::vector<uint8_t> prior;
    if (!rd(f, off, (size_t)B + 1) || !rd(f, soff, (size_t)B + 1) || !rd(f, prob, (size_t)B)) return 1;
    if (off[0] != 0 || soff[0] != 0) return 1;
    for (int b = 0; b < B; b++)
        if (off[b + 1] < off[b] || soff[b + 1] < soff[b] || off[b + 1] > (1 << 20) || soff[b + 1] > (1 << 20) ||
            (soff[b + 1] > soff[b] && (off[b + 1] - off[b] < 4 || off[b + 1] - off[b] < prob[b].min_inliers))) return 1;
    const int np = off[B], nh = soff[B], ns = nh + B;
    if (!rd(f, corrs, (size_t)np) || !rd(f, sets, (size_t)nh * 4) || !rd(f, prior, (size_t)np)) return 1;
    fclose(f);
    std::vector<int64_t> fbase(B + 1), rbase(B + 1);
    hprob.assign(nh + 1, 0); rprob.assign(ns + 1, 0);
    int64_t fb = 0, rb = 0;
    for (int b = 0; b < B; b++) {
        const int n = off[b + 1] - off[b], its = soff[b + 1] - soff[b];
        fbase[b] = fb; rbase[b] = rb;
        for (int h = soff[b]; h < soff[b + 1]; h++) {
            hprob[h] = b;
            for (int c = 0; c < 4; c++)
                if (sets[h * 4 + c] < 0 || sets[h * 4 + c] >= n) return 1;
        }
        for (int k = 0; k <= its; k++) rprob[soff[b] + b + k] = b;
        fb += (int64_t)its * n; rb += (int64_t)(its + 1) * n;
    }
    PnpIn in;
    in.corrs = corrs.data(); in.prob = prob.data(); in.off = off.data(); in.soff = soff.data(); in.sets = sets.data();
    in.hprob = hprob.data(); in.rprob = rprob.data(); in.fbase = fbase.data(); in.rbase = rbase.data(); in.prior = prior.data();
    in.B = B; in.ncorr = np; in.nhyp = nh;
    std::vector<double> models((size_t)nh * 12 + 1), rmodels((size_t)ns * 12 + 1), points((size_t)rb * PNP_PT + 1);
    std::vector<float> tcws((size_t)nh * 16 + 1), rtcws((size_t)ns * 16 + 1);
    std::vector<int32_t> counts(nh + 1), choices(nh + 1), rcounts(ns + 1, -1);
    std::vector<uint8_t> flags((size_t)fb + 1), rflags((size_t)rb + 1), inl(np + 1), best(np + 1);
    std::vector<orbp_pnp_info_t> infos(B);
    memset(infos.data(), 0, B * sizeof(orbp_pnp_info_t));
    if (nh > 0) {
        for (blockIdx.x = 0; blockIdx.x < nh; blockIdx.x++) k_pnp_ransac(in, models.data(), tcws.data(), choices.data(), counts.data(), flags.data());
        for (blockIdx.x = 0; blockIdx.x < ns; blockIdx.x++)
            k_pnp_refine(in, counts.data(), flags.data(), points.data(), rmodels.data(), rtcws.data(), rcounts.data(), rflags.data());
    }
    for (blockIdx.x = 0; blockIdx.x < B; blockIdx.x++)
        k_pnp_select(in, tcws.data(), counts.data(), flags.data(), rtcws.data(), rcounts.data(), rflags.data(), inl.data(), best.data(), infos.data());
    f = fopen(argv[2], "wb");
    if (!f) return 1;
    fwrite(infos.data(), sizeof(orbp_pnp_info_t), B, f); fwrite(counts.data(), 4, nh, f); fwrite(choices.data(), 4, nh, f);
    fwrite(rcounts.data(), 4, ns, f); fwrite(inl.data(), 1, np, f); fwrite(best.data(), 1, np, f);
    fwrite(models.data(), 8, (size_t)nh * 12, f); fwrite(tcws.data(), 4, (size_t)nh * 16, f);
    fwrite(rmodels.data(), 8, (size_t)ns * 12, f); fwrite(rtcws.data(), 4, (size_t)ns * 16, f);
    fwrite(flags.data(), 1, (size_t)fb, f); fwrite(rflags.data(), 1, (size_t)rb, f);
    fclose(f);
    return 0;
}
