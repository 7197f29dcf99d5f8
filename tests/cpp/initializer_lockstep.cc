// initializer_lockstep.cc — the text of k_init_normalize / k_init_ransac / k_init_select / k_init_reconstruct
// (orb_slam2v2-1_amd/csrc/orbx_initializer.hip) compiled for the host and run as ONE thread per workgroup, the workgroups one
// after the other, for tests/test_initializer_cpu.py: every output byte must equal tests/init_ref.py's.  That pins the kernels'
// arithmetic and control flow without a GPU; what it cannot show - the sharing of rows and matches among threads, the barriers,
// the device's division, sqrt and acosf - is tests/test_initializer_gpu.py's.  Build with -ffp-contract=off, as the library is.
//   initializer_lockstep IN OUT [REPEAT]
//       IN:  int32 n1 n2 N iterations | float fx fy cx cy sigma minParallax | int32 minTriangulated |
//            float keys1[n1][2] | float keys2[n2][2] | int32 matches[N][2] | int32 sets[iterations][8]
//       OUT: orbi_init_info_t | int32 result | float R21[9] t21[3] | float scores[2][iterations] | uint8 inliersH[N] inliersF[N] |
//            float P3D[N][3] | uint8 triangulated[N]
//       REPEAT > 1 runs the chain that many times and prints the seconds per run (the single-core host figure of profiles/README.md)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <vector>
#include "orbx.h"

#define ORBX_INIT_HOST
#include "hip_lockstep.h"

#include "orbx_initializer.hip"

template <typename T> static bool rd(FILE *f, std::vector<T> &v, size_t n) { v.resize(n + 1); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: initializer_lockstep IN OUT [REPEAT]\n"); return 2; }
    const int repeat = argc > 3 ? atoi(argv[3]) : 1;
    FILE *f = fopen(argv[1], "rb");
    int32_t hd[4], minTri;
    float fl[6];
    if (!f || fread(hd, 4, 4, f) != 4 || fread(fl, 4, 6, f) != 6 || fread(&minTri, 4, 1, f) != 1) return 1;
    const int n1 = hd[0], n2 = hd[1], N = hd[2], iters = hd[3];
    if (n1 < 1 || n2 < 1 || N < 8 || iters < 1) return 1;
    std::vector<float> k1, k2;
    std::vector<int32_t> matches, sets;
    if (!rd(f, k1, (size_t)n1 * 2) || !rd(f, k2, (size_t)n2 * 2) || !rd(f, matches, (size_t)N * 2) || !rd(f, sets, (size_t)iters * 8)) return 1;
    fclose(f);
    for (int i = 0; i < N; i++)
        if (matches[2 * i] < 0 || matches[2 * i] >= n1 || matches[2 * i + 1] < 0 || matches[2 * i + 1] >= n2) return 1;
    for (int i = 0; i < iters * 8; i++)
        if (sets[i] < 0 || sets[i] >= N) return 1;
    InitIn in;
    in.k1 = k1.data(); in.k2 = k2.data(); in.s1 = in.s2 = 2; in.n1 = n1; in.n2 = n2; in.matches = matches.data(); in.N = N;
    in.sets = sets.data(); in.iters = iters; in.fx = fl[0]; in.fy = fl[1]; in.cx = fl[2]; in.cy = fl[3]; in.sigma = fl[4];
    in.minParallax = fl[5]; in.minTri = minTri;
    const size_t nh = 2 * (size_t)iters;
    InitNorm norm;
    std::vector<float> models(nh * 9), scores(nh), candP(8 * (size_t)N * 3), candC(8 * (size_t)N), P3D((size_t)N * 3);
    std::vector<uint8_t> inl(nh * N), inlBest(2 * (size_t)N), candF(8 * (size_t)N), tri(N);
    orbi_init_info_t info;
    InitOut out;
    const clock_t t0 = clock();
    for (int r = 0; r < repeat; r++) {
        memset(&info, 0, sizeof(info)); memset(&out, 0, sizeof(out)); memset(&norm, 0, sizeof(norm));
        for (blockIdx.x = 0; blockIdx.x < 2; blockIdx.x++) k_init_normalize(in, &norm);
        for (blockIdx.x = 0; blockIdx.x < (int)nh; blockIdx.x++) k_init_ransac(in, &norm, models.data(), scores.data(), inl.data());
        blockIdx.x = 0;
        k_init_select(in, models.data(), scores.data(), inl.data(), inlBest.data(), &info);
        k_init_reconstruct(in, inlBest.data(), candP.data(), candF.data(), candC.data(), &info, &out, P3D.data(), tri.data());
    }
    if (repeat > 1) printf("%.6f\n", (double)(clock() - t0) / CLOCKS_PER_SEC / repeat);
    f = fopen(argv[2], "wb");
    if (!f) return 1;
    fwrite(&info, sizeof(info), 1, f); fwrite(&out.result, 4, 1, f); fwrite(out.R, 4, 9, f); fwrite(out.t, 4, 3, f);
    fwrite(scores.data(), 4, nh, f); fwrite(inlBest.data(), 1, 2 * (size_t)N, f); fwrite(P3D.data(), 4, (size_t)N * 3, f);
    fwrite(tri.data(), 1, N, f);
    fclose(f);
    return 0;
}
