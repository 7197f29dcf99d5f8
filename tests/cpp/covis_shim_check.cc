// covis_shim_check.cc — host/frame_shim.h's MapPoint::UpdateNormalAndDepth on objects built from an observation table, for
// tests/test_covis_cpu.py: what it writes must equal tests/covis_ref.py's restatement (and so the kernel's text) in every bit.
// The keyframes live in one array, so the pointer order of a point's std::map is the table's slot order.  A point whose reference
// keyframe is set but not among its observers is not passed to the shim (observations[pRefKF] inserts there, as in the reference).
//   covis_shim_check IN OUT
//       IN:  int32 K P nobs nlevels | orbc_keyframe_t[K] | orbc_point_t[P] | int32 obs_off[P+1] | orbc_observation_t[nobs] | float sf[nlevels]
//       OUT: per point float normal[3], max_distance, min_distance
#include <stdio.h>
#include <vector>
#include "frame_shim.h"
#include "orbx.h"

using namespace ORB_SLAM2;

template <typename T> static bool rd(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n + 1);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: covis_shim_check IN OUT\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    int32_t hd[4];
    if (!f || fread(hd, 4, 4, f) != 4) return 1;
    const int K = hd[0], P = hd[1], nobs = hd[2], nlevels = hd[3];
    std::vector<orbc_keyframe_t> kf;
    std::vector<orbc_point_t> pts;
    std::vector<int32_t> off;
    std::vector<orbc_observation_t> obs;
    std::vector<float> sf;
    if (!rd(f, kf, K) || !rd(f, pts, P) || !rd(f, off, P + 1) || !rd(f, obs, nobs) || !rd(f, sf, nlevels)) return 1;
    fclose(f);
    sf.resize(nlevels);
    std::vector<KeyFrame> kfs(K);
    for (int s = 0; s < K; s++) {
        kfs[s].mnId = (long unsigned int)kf[s].id;
        kfs[s].Ow = cv::Mat(3, 1, CV_32F);
        for (int c = 0; c < 3; c++) kfs[s].Ow.at<float>(c) = kf[s].Ow[c];
        kfs[s].mvScaleFactors = sf; kfs[s].mnScaleLevels = nlevels;
    }
    for (int o = 0; o < nobs; o++) {
        KeyFrame &k = kfs[obs[o].kf];
        if ((int)k.mvKeysUn.size() <= obs[o].idx) k.mvKeysUn.resize(obs[o].idx + 1);
        k.mvKeysUn[obs[o].idx].octave = obs[o].octave;
    }
    std::vector<MapPoint> mps(P);
    f = fopen(argv[2], "wb");
    if (!f) return 1;
    for (int p = 0; p < P; p++) {
        MapPoint &m = mps[p];
        for (int c = 0; c < 3; c++) m.mWorldPos.at<float>(c) = pts[p].pos[c];
        m.mbBad = pts[p].bad != 0;
        m.mpRefKF = pts[p].ref_kf >= 0 ? &kfs[pts[p].ref_kf] : NULL;
        for (int o = off[p]; o < off[p + 1]; o++) m.mObservations[&kfs[obs[o].kf]] = (size_t)obs[o].idx;
        if (!m.mpRefKF || m.mObservations.count(m.mpRefKF)) m.UpdateNormalAndDepth();
        const float out[5] = {m.mNormalVector.at<float>(0), m.mNormalVector.at<float>(1), m.mNormalVector.at<float>(2), m.mfMaxDistance, m.mfMinDistance};
        fwrite(out, 4, 5, f);
    }
    fclose(f);
    return 0;
}
