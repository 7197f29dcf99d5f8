// mapcorrect_host_loops.cc — the two map-sized loops of LoopClosing as the reference writes them (src/LoopClosing.cc:457-525 without the
// UpdateConnections of :524, and :685-746), on the CPU over host/frame_shim.h's objects, std::maps and cv::Mat temporaries, for
// tools/bench_mapcorrect.py: what the device calls are measured against.  One thread, the best of REPS runs; the objects are rebuilt
// before every run and only the loops are timed.
//   mapcorrect_host_loops loop|spread IN REPS      IN: the input format of tests/cpp/mapcorrect_lockstep.cc
//   prints one JSON object: {"ms": best, "pos_sum": the sum of every point's coordinates after the loops, in double}
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <vector>
#include "frame_shim.h"
#include "g2o_shim.h"
#include "orbx.h"

using namespace ORB_SLAM2;

template <typename T> static bool rd(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n + 1);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
static cv::Mat mat44(const float *p) {
    cv::Mat T(4, 4, CV_32F);
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) T.at<float>(r, c) = p[r * 4 + c];
    return T;
}
// cv::Mat products as the reference's expressions make them: a new matrix per operation
static cv::Mat mul44(const cv::Mat &a, const cv::Mat &b) {
    cv::Mat d(4, 4, CV_32F);
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double s = 0;
            for (int k = 0; k < 4; k++) s += (double)a.at<float>(i, k) * (double)b.at<float>(k, j);
            d.at<float>(i, j) = (float)s;
        }
    return d;
}
static cv::Mat pose_inverse(KeyFrame *k) {   // GetPoseInverse(): the Twc SetPose keeps
    cv::Mat T = k->GetPose(), O = k->GetCameraCenter(), Twc = cv::Mat::eye(4, 4, CV_32F);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) Twc.at<float>(r, c) = T.at<float>(c, r);
        Twc.at<float>(r, 3) = O.at<float>(r);
    }
    return Twc;
}
static cv::Mat rot_add(const cv::Mat &T, bool transposed, const cv::Mat &x, const cv::Mat &t) {   // R * x + t, R the top-left block of T (or its transpose)
    cv::Mat d(3, 1, CV_32F);
    for (int i = 0; i < 3; i++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)(transposed ? T.at<float>(k, i) : T.at<float>(i, k)) * (double)x.at<float>(k);
        d.at<float>(i) = (float)(s + (double)t.at<float>(i));
    }
    return d;
}
static g2o::Sim3 sim3_of(const cv::Mat &T) {
    cv::Mat R(3, 3, CV_32F), t(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) R.at<float>(r, c) = T.at<float>(r, c);
        t.at<float>(r) = T.at<float>(r, 3);
    }
    return g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), 1.0);
}
static double pos_sum(std::vector<MapPoint> &mps) {
    double s = 0;
    for (size_t p = 0; p < mps.size(); p++)
        for (int c = 0; c < 3; c++) s += (double)mps[p].mWorldPos.at<float>(c);
    return s;
}
typedef std::chrono::steady_clock Clock;

static int run_loop(FILE *f, int reps) {
    int32_t hd[7];
    if (fread(hd, 4, 7, f) != 7) return 1;
    const int K = hd[0], P = hd[1], nobs = hd[2], nlevels = hd[3], Q = hd[4], nfeat = hd[5], cur = hd[6];
    std::vector<orbc_keyframe_t> kf;
    std::vector<orbc_point_t> pts;
    std::vector<int32_t> off, qk, foff;
    std::vector<orbc_observation_t> obs;
    std::vector<float> sf, Tiw;
    std::vector<orbc_feature_t> feat;
    std::vector<orbg_sim3_t> Scw;
    if (!rd(f, kf, K) || !rd(f, pts, P) || !rd(f, off, P + 1) || !rd(f, obs, nobs) || !rd(f, sf, nlevels) || !rd(f, qk, Q) || !rd(f, foff, Q + 1) ||
        !rd(f, feat, nfeat) || !rd(f, Tiw, (size_t)Q * 16) || !rd(f, Scw, 1)) return 1;
    sf.resize(nlevels);
    double best = 1e300, sum = 0;
    for (int rep = 0; rep < reps; rep++) {
        std::vector<KeyFrame> kfs(K);
        std::vector<MapPoint> mps(P);
        std::vector<size_t> nk(K, 0);
        for (int o = 0; o < nobs; o++) nk[obs[o].kf] = std::max(nk[obs[o].kf], (size_t)obs[o].idx + 1);
        for (int s = 0; s < K; s++) {
            kfs[s].mnId = (long unsigned int)s + 1; kfs[s].mvScaleFactors = sf; kfs[s].mnScaleLevels = nlevels;
            kfs[s].mvKeysUn.resize(nk[s]); kfs[s].mvuRight.assign(nk[s], -1.f);
            for (int c = 0; c < 3; c++) kfs[s].Ow.at<float>(c) = kf[s].Ow[c];
        }
        for (int p = 0; p < P; p++) {
            mps[p].mbBad = pts[p].bad; mps[p].mpRefKF = pts[p].ref_kf >= 0 ? &kfs[pts[p].ref_kf] : NULL;
            for (int c = 0; c < 3; c++) mps[p].mWorldPos.at<float>(c) = pts[p].pos[c];
            for (int o = off[p]; o < off[p + 1]; o++) {
                kfs[obs[o].kf].mvKeysUn[obs[o].idx].octave = obs[o].octave;
                mps[p].mObservations[&kfs[obs[o].kf]] = (size_t)obs[o].idx;
            }
        }
        std::vector<KeyFrame *> connected;
        for (int q = 0; q < Q; q++) {
            KeyFrame *k = &kfs[qk[q]];
            k->SetPose(mat44(&Tiw[(size_t)q * 16]));
            k->mvpMapPoints.assign(foff[q + 1] - foff[q], static_cast<MapPoint *>(NULL));
            for (int i = foff[q]; i < foff[q + 1]; i++)
                if (feat[i].point >= 0) k->mvpMapPoints[i - foff[q]] = &mps[feat[i].point];
            connected.push_back(k);
        }
        KeyFrame *pCur = &kfs[cur];
        const g2o::Sim3 g2oScw(Eigen::Quaterniond(Scw[0].q[3], Scw[0].q[0], Scw[0].q[1], Scw[0].q[2]), Eigen::Vector3d(Scw[0].t[0], Scw[0].t[1], Scw[0].t[2]), Scw[0].s);
        const Clock::time_point t0 = Clock::now();
        LoopClosing::KeyFrameAndPose CorrectedSim3, NonCorrectedSim3;
        CorrectedSim3[pCur] = g2oScw;
        cv::Mat Twc = pose_inverse(pCur);
        for (size_t i = 0; i < connected.size(); i++) {   // :457-479
            KeyFrame *pKFi = connected[i];
            cv::Mat T = pKFi->GetPose();
            if (pKFi != pCur) CorrectedSim3[pKFi] = sim3_of(mul44(T, Twc)) * g2oScw;
            NonCorrectedSim3[pKFi] = sim3_of(T);
        }
        for (LoopClosing::KeyFrameAndPose::iterator mit = CorrectedSim3.begin(), mend = CorrectedSim3.end(); mit != mend; mit++) {   // :482-525
            KeyFrame *pKFi = mit->first;
            g2o::Sim3 g2oCorrectedSiw = mit->second, g2oCorrectedSwi = g2oCorrectedSiw.inverse(), g2oSiw = NonCorrectedSim3[pKFi];
            std::vector<MapPoint *> vpMPsi = pKFi->GetMapPointMatches();
            for (size_t iMP = 0, endMPi = vpMPsi.size(); iMP < endMPi; iMP++) {
                MapPoint *pMPi = vpMPsi[iMP];
                if (!pMPi) continue;
                if (pMPi->isBad()) continue;
                if (pMPi->mnCorrectedByKF == pCur->mnId) continue;
                cv::Mat P3Dw = pMPi->GetWorldPos();
                Eigen::Vector3d c = g2oCorrectedSwi.map(g2oSiw.map(Converter::toVector3d(P3Dw)));
                cv::Mat cv3(3, 1, CV_32F);
                for (int k = 0; k < 3; k++) cv3.at<float>(k) = (float)c[k];
                pMPi->SetWorldPos(cv3);
                pMPi->mnCorrectedByKF = pCur->mnId;
                pMPi->mnCorrectedReference = pKFi->mnId;
                if (pMPi->mpRefKF && pMPi->mObservations.count(pMPi->mpRefKF)) pMPi->UpdateNormalAndDepth();
            }
            Eigen::Matrix3d eigR = g2oCorrectedSiw.rotation().toRotationMatrix();
            Eigen::Vector3d eigt = g2oCorrectedSiw.translation();
            const double s = 1. / g2oCorrectedSiw.scale();
            cv::Mat correctedTiw = cv::Mat::eye(4, 4, CV_32F);
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) correctedTiw.at<float>(r, c) = (float)eigR(r, c);
                correctedTiw.at<float>(r, 3) = (float)(eigt[r] * s);
            }
            pKFi->SetPose(correctedTiw);
        }
        const double ms = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
        if (ms < best) best = ms;
        sum = pos_sum(mps);
    }
    printf("{\"ms\": %.4f, \"pos_sum\": %.17g}\n", best, sum);
    return 0;
}

static int run_spread(FILE *f, int reps) {
    int32_t hd[4];
    if (fread(hd, 4, 4, f) != 4) return 1;
    const int K = hd[0], P = hd[1], nchild = hd[2], norigins = hd[3];
    std::vector<float> Tcw, gba, pos, posg;
    std::vector<uint8_t> ingba, ptin, bad;
    std::vector<int32_t> coff, child, origins, refkf;
    if (!rd(f, Tcw, (size_t)K * 16) || !rd(f, gba, (size_t)K * 16) || !rd(f, ingba, K) || !rd(f, coff, K + 1) || !rd(f, child, nchild) || !rd(f, origins, norigins) ||
        !rd(f, pos, (size_t)P * 3) || !rd(f, posg, (size_t)P * 3) || !rd(f, ptin, P) || !rd(f, refkf, P) || !rd(f, bad, P)) return 1;
    const unsigned long nLoopKF = 77;
    double best = 1e300, sum = 0;
    for (int rep = 0; rep < reps; rep++) {
        std::vector<KeyFrame> kfs(K);
        std::vector<MapPoint> mps(P);
        Map map;
        for (int s = 0; s < K; s++) {
            kfs[s].mnId = (long unsigned int)s + 1;
            kfs[s].SetPose(mat44(&Tcw[(size_t)s * 16]));
            if (ingba[s]) { kfs[s].mTcwGBA = mat44(&gba[(size_t)s * 16]); kfs[s].mnBAGlobalForKF = nLoopKF; }
            for (int i = coff[s]; i < coff[s + 1]; i++) kfs[s].mspChildrens.insert(&kfs[child[i]]);
        }
        for (int i = 0; i < norigins; i++) map.mvpKeyFrameOrigins.push_back(&kfs[origins[i]]);
        for (int p = 0; p < P; p++) {
            mps[p].mbBad = bad[p]; mps[p].mpRefKF = refkf[p] >= 0 ? &kfs[refkf[p]] : NULL;
            mps[p].mPosGBA = cv::Mat(3, 1, CV_32F);
            for (int c = 0; c < 3; c++) { mps[p].mWorldPos.at<float>(c) = pos[(size_t)p * 3 + c]; mps[p].mPosGBA.at<float>(c) = posg[(size_t)p * 3 + c]; }
            if (ptin[p]) mps[p].mnBAGlobalForKF = nLoopKF;
            map.AddMapPoint(&mps[p]);
        }
        const Clock::time_point t0 = Clock::now();
        std::list<KeyFrame *> lpKFtoCheck(map.mvpKeyFrameOrigins.begin(), map.mvpKeyFrameOrigins.end());   // :686-709
        while (!lpKFtoCheck.empty()) {
            KeyFrame *pKF = lpKFtoCheck.front();
            const std::set<KeyFrame *> sChilds = pKF->GetChilds();
            cv::Mat Twc = pose_inverse(pKF);
            for (std::set<KeyFrame *>::const_iterator sit = sChilds.begin(); sit != sChilds.end(); sit++) {
                KeyFrame *pChild = *sit;
                if (pChild->mnBAGlobalForKF != nLoopKF) {
                    cv::Mat Tchildc = mul44(pChild->GetPose(), Twc);
                    pChild->mTcwGBA = mul44(Tchildc, pKF->mTcwGBA);
                    pChild->mnBAGlobalForKF = nLoopKF;
                }
                lpKFtoCheck.push_back(pChild);
            }
            pKF->mTcwBefGBA = pKF->GetPose();
            pKF->SetPose(pKF->mTcwGBA);
            lpKFtoCheck.pop_front();
        }
        const std::vector<MapPoint *> vpMPs = map.GetAllMapPoints();   // :712-746
        for (size_t i = 0; i < vpMPs.size(); i++) {
            MapPoint *pMP = vpMPs[i];
            if (pMP->isBad()) continue;
            if (pMP->mnBAGlobalForKF == nLoopKF) pMP->SetWorldPos(pMP->mPosGBA);
            else {
                KeyFrame *pRefKF = pMP->GetReferenceKeyFrame();
                if (!pRefKF || pRefKF->mnBAGlobalForKF != nLoopKF || pRefKF->mTcwBefGBA.empty()) continue;
                cv::Mat tcw(3, 1, CV_32F);
                for (int c = 0; c < 3; c++) tcw.at<float>(c) = pRefKF->mTcwBefGBA.at<float>(c, 3);
                cv::Mat Xc = rot_add(pRefKF->mTcwBefGBA, false, pMP->GetWorldPos(), tcw);
                pMP->SetWorldPos(rot_add(pRefKF->GetPose(), true, Xc, pRefKF->GetCameraCenter()));
            }
        }
        const double ms = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
        if (ms < best) best = ms;
        sum = pos_sum(mps);
    }
    printf("{\"ms\": %.4f, \"pos_sum\": %.17g}\n", best, sum);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "usage: mapcorrect_host_loops loop|spread IN REPS\n"); return 2; }
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 1;
    const int reps = atoi(argv[3]);
    const int rc = !strcmp(argv[1], "loop") ? run_loop(f, reps) : !strcmp(argv[1], "spread") ? run_spread(f, reps) : 2;
    fclose(f);
    return rc;
}
