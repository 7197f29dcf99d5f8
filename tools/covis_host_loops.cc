// covisibility on the CPU, for tools/bench_covis.py's yardstick column: what KeyFrame::UpdateConnections (src/KeyFrame.cc:290-380),
// LocalMapping::KeyFrameCulling (src/LocalMapping.cc:640-704) and MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:340-383) compute, over
// host/frame_shim.h's objects with their std::map<KeyFrame*, size_t> observation lists.  The normals ARE the shim's own
// MapPoint::UpdateNormalAndDepth and the erasing is the shim's KeyFrame::SetBadFlag; the two loops around them are written here in
// this project's own words, keeping only what decides their cost: one std::map per keyframe for the counts, and a copy of a point's
// observation map per visit.  Input: the IN file of tests/cpp/covis_lockstep.cc.  Prints one JSON line of milliseconds (the best of
// REPS runs each; culling changes its objects and so runs once per rebuild of them) and three checksums, which bench_covis.py
// compares with the device's results.
//   g++ -std=c++11 -O2 -I include -I orb_slam2v2-1_amd/host tools/covis_host_loops.cc -o covis_host_loops
#include <chrono>
#include <cstdio>
#include <vector>
#include "frame_shim.h"
#include "orbx.h"

using namespace ORB_SLAM2;
typedef std::chrono::steady_clock Clock;
static double ms(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

template <typename T> static bool rd(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n + 1);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

struct World {
    std::vector<KeyFrame> kfs;
    std::vector<MapPoint> mps;
};

// The covisibility list of one keyframe: how many of its good points each other keyframe sees, the ones at 15 or more (or the single
// best one) by falling (weight, pointer).  The per-point copy of the observation map is the cost the reference pays (GetObservations
// returns by value), so it is paid here too
static long connections_of(KeyFrame *self) {
    std::map<KeyFrame *, int> shared;
    const std::vector<MapPoint *> points = self->mvpMapPoints;
    for (MapPoint *pt : points) {
        if (!pt || pt->mbBad) continue;
        const std::map<KeyFrame *, size_t> seen = pt->GetObservations();
        for (const std::pair<KeyFrame *const, size_t> &e : seen)
            if (e.first->mnId != self->mnId) ++shared[e.first];
    }
    if (shared.empty()) return 0;
    std::vector<std::pair<int, KeyFrame *> > strong;
    std::pair<int, KeyFrame *> best(0, static_cast<KeyFrame *>(NULL));
    for (const std::pair<KeyFrame *const, int> &e : shared) {
        if (e.second > best.first) best = std::make_pair(e.second, e.first);
        if (e.second >= 15) strong.push_back(std::make_pair(e.second, e.first));
    }
    if (strong.empty()) strong.push_back(best);
    std::sort(strong.rbegin(), strong.rend());
    self->mConnectedKeyFrameWeights = shared;
    self->mvpOrderedConnectedKeyFrames.clear(); self->mvOrderedWeights.clear();
    for (const std::pair<int, KeyFrame *> &e : strong) { self->mvpOrderedConnectedKeyFrames.push_back(e.second); self->mvOrderedWeights.push_back(e.first); }
    return (long)strong.size() + strong.front().first;
}

// at least `need` other keyframes see the point at the feature's level + 1 or finer (the map is copied, as above)
static bool seen_well_elsewhere(MapPoint *pt, KeyFrame *self, int level, int need) {
    const std::map<KeyFrame *, size_t> seen = pt->GetObservations();
    int hits = 0;
    for (const std::pair<KeyFrame *const, size_t> &e : seen) {
        if (e.first == self || e.first->mvKeysUn[e.second].octave > level + 1) continue;
        if (++hits >= need) return true;
    }
    return hits >= need;
}

// the local keyframes in order; one whose usable points are more than 90 % seen well elsewhere is erased before the next is looked at
static long cull_in_order(const std::vector<KeyFrame *> &local, bool monocular) {
    const int need = 3;
    long erased = 0;
    for (KeyFrame *kf : local) {
        if (kf->mnId == 0) continue;
        const std::vector<MapPoint *> points = kf->GetMapPointMatches();
        int usable = 0, covered = 0;
        for (size_t i = 0; i < points.size(); i++) {
            MapPoint *pt = points[i];
            if (!pt || pt->isBad()) continue;
            if (!monocular && (kf->mvDepth[i] > kf->mThDepth || kf->mvDepth[i] < 0)) continue;
            usable++;
            if (pt->Observations() > need && seen_well_elsewhere(pt, kf, kf->mvKeysUn[i].octave, need)) covered++;
        }
        if (covered > 0.9 * usable) { kf->SetBadFlag(); erased++; }
    }
    return erased;
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: covis_host_loops IN [REPS]\n"); return 2; }
    const int reps = argc > 2 ? atoi(argv[2]) : 3;
    FILE *f = fopen(argv[1], "rb");
    int32_t hd[12];
    if (!f || fread(hd, 4, 12, f) != 12) return 1;
    const int K = hd[0], P = hd[1], nobs = hd[2], nlevels = hd[3], Qc = hd[4], Fc = hd[5], Qk = hd[6], Fk = hd[7], monocular = hd[10];
    std::vector<orbc_keyframe_t> kf;
    std::vector<orbc_point_t> pts;
    std::vector<int32_t> off, cq, coff, kq, koff;
    std::vector<orbc_observation_t> obs;
    std::vector<float> sf;
    std::vector<orbc_feature_t> cfeat, kfeat;
    if (!rd(f, kf, K) || !rd(f, pts, P) || !rd(f, off, P + 1) || !rd(f, obs, nobs) || !rd(f, sf, nlevels) || !rd(f, cq, Qc) || !rd(f, coff, Qc + 1) ||
        !rd(f, cfeat, Fc) || !rd(f, kq, Qk) || !rd(f, koff, Qk + 1) || !rd(f, kfeat, Fk)) return 1;
    fclose(f);
    sf.resize(nlevels);
    auto build = [&](World &W, const std::vector<int32_t> &qk, const std::vector<int32_t> &qoff, const std::vector<orbc_feature_t> &qf, int Q) {
        W.kfs = std::vector<KeyFrame>(K);
        W.mps = std::vector<MapPoint>(P);
        std::vector<int> nfeat(K, 0);
        for (int o = 0; o < nobs; o++) if (nfeat[obs[o].kf] <= obs[o].idx) nfeat[obs[o].kf] = obs[o].idx + 1;
        for (int q = 0; q < Q; q++) if (nfeat[qk[q]] < qoff[q + 1] - qoff[q]) nfeat[qk[q]] = qoff[q + 1] - qoff[q];
        for (int s = 0; s < K; s++) {
            KeyFrame &k = W.kfs[s];
            k.mnId = (long unsigned int)kf[s].id; k.mbNotErase = kf[s].not_erase; k.mThDepth = kf[s].th_depth;
            k.Ow = cv::Mat(3, 1, CV_32F);
            for (int c = 0; c < 3; c++) k.Ow.at<float>(c) = kf[s].Ow[c];
            k.mvScaleFactors = sf; k.mnScaleLevels = nlevels;
            k.mvKeysUn.resize(nfeat[s]); k.mvuRight.assign(nfeat[s], -1.f); k.mvDepth.assign(nfeat[s], -1.f); k.mvpMapPoints.assign(nfeat[s], static_cast<MapPoint *>(NULL));
        }
        for (int p = 0; p < P; p++) {
            MapPoint &m = W.mps[p];
            for (int c = 0; c < 3; c++) m.mWorldPos.at<float>(c) = pts[p].pos[c];
            m.mbBad = pts[p].bad != 0; m.mpRefKF = pts[p].ref_kf >= 0 ? &W.kfs[pts[p].ref_kf] : NULL;
            for (int o = off[p]; o < off[p + 1]; o++) {
                KeyFrame &k = W.kfs[obs[o].kf];
                k.mvKeysUn[obs[o].idx].octave = obs[o].octave; k.mvuRight[obs[o].idx] = obs[o].stereo ? 1.f : -1.f; k.mvpMapPoints[obs[o].idx] = &m;
                m.AddObservation(&k, (size_t)obs[o].idx);
            }
        }
        for (int q = 0; q < Q; q++) {
            KeyFrame &k = W.kfs[qk[q]];
            for (int i = qoff[q]; i < qoff[q + 1]; i++) {
                const int j = i - qoff[q];
                k.mvpMapPoints[j] = qf[i].point >= 0 ? &W.mps[qf[i].point] : NULL; k.mvKeysUn[j].octave = qf[i].octave; k.mvDepth[j] = qf[i].depth;
            }
        }
    };
    double tConn = 1e30, tCull = 1e30, tNorm = 1e30;
    long sConn = 0, sCull = 0;
    double sNorm = 0;
    for (int r = 0; r < reps; r++) {
        World W;
        build(W, cq, coff, cfeat, Qc);
        Clock::time_point a = Clock::now();
        sConn = 0;
        for (int q = 0; q < Qc; q++) sConn += connections_of(&W.kfs[cq[q]]);
        Clock::time_point b = Clock::now();
        if (Qc && ms(a, b) < tConn) tConn = ms(a, b);
        a = Clock::now();
        sNorm = 0;
        for (int p = 0; p < P; p++) {
            MapPoint &m = W.mps[p];
            if (!m.mpRefKF || m.mObservations.count(m.mpRefKF)) m.UpdateNormalAndDepth();
            sNorm += m.mfMaxDistance;
        }
        b = Clock::now();
        if (P && ms(a, b) < tNorm) tNorm = ms(a, b);
        World V;
        build(V, kq, koff, kfeat, Qk);
        std::vector<KeyFrame *> local(Qk);
        for (int q = 0; q < Qk; q++) local[q] = &V.kfs[kq[q]];
        a = Clock::now();
        sCull = cull_in_order(local, monocular != 0);
        b = Clock::now();
        if (Qk && ms(a, b) < tCull) tCull = ms(a, b);
    }
    printf("{\"host_connections_ms\": %.4f, \"host_culling_ms\": %.4f, \"host_normals_ms\": %.4f, \"connections_sum\": %ld, \"culled\": %ld, \"max_distance_sum\": %.12g}\n",
           Qc ? tConn : 0.0, Qk ? tCull : 0.0, P ? tNorm : 0.0, sConn, sCull, sNorm);
    return 0;
}
