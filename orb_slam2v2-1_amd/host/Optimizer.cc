// Optimizer.cc — see Optimizer.h.
#include "Optimizer.h"
#include <cstdlib>
#include <stdexcept>
#include <string>
#include "orbx.h"

namespace ORB_SLAM2 {

int Optimizer::device = std::getenv("ORBX_DEVICE") ? std::atoi(std::getenv("ORBX_DEVICE")) : 0;

int Optimizer::PoseOptimization(Frame *pFrame) {
    const int N = pFrame->N;
    std::vector<orbo_observation_t> obs((size_t)N);
    std::vector<uint8_t> outlier((size_t)N);
    for (int i = 0; i < N; i++) {
        orbo_observation_t &o = obs[i];
        MapPoint *pMP = pFrame->mvpMapPoints[i];
        outlier[i] = pFrame->mvbOutlier[i] ? 1 : 0;
        o.valid = pMP ? 1 : 0;
        const cv::KeyPoint &kpUn = pFrame->mvKeysUn[i];
        o.u = kpUn.pt.x; o.v = kpUn.pt.y; o.ur = pFrame->mvuRight[i];
        o.inv_sigma2 = pFrame->mvInvLevelSigma2[kpUn.octave];
        o.wx = o.wy = o.wz = 0.f;
        if (pMP) {
            cv::Mat Xw = pMP->GetWorldPos();
            o.wx = Xw.at<float>(0); o.wy = Xw.at<float>(1); o.wz = Xw.at<float>(2);
        }
    }
    const orbm_camera_t cam = {pFrame->fx, pFrame->fy, pFrame->cx, pFrame->cy, pFrame->mbf, pFrame->mb};
    float Tin[16], Tout[16];
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) Tin[r * 4 + c] = pFrame->mTcw.at<float>(r, c);
    int ngood = 0;
    orbo_pose_info_t info;
    const int rc = orbo_pose_optimization(obs.data(), N, &cam, Tin, Tout, outlier.data(), &ngood, &info, device);
    if (rc != ORBX_OK) throw std::runtime_error(std::string("Optimizer::PoseOptimization: ") + orbx_last_error());
    for (int i = 0; i < N; i++)
        if (obs[i].valid) pFrame->mvbOutlier[i] = outlier[i] != 0;
    if (info.correspondences < 3) return 0;   // :364-365: returns before the pose is written
    cv::Mat pose(4, 4, CV_32F);
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) pose.at<float>(r, c) = Tout[r * 4 + c];
    pFrame->SetPose(pose);
    return ngood;
}

int Optimizer::OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches1, g2o::Sim3 &g2oS12, const float th2,
                            const bool bFixScale) {
    orbz_sim3_problem_t prob;
    const cv::Mat &K1 = pKF1->mK;
    const cv::Mat &K2 = pKF2->mK;
    prob.K1[0] = K1.at<float>(0, 0); prob.K1[1] = K1.at<float>(1, 1); prob.K1[2] = K1.at<float>(0, 2); prob.K1[3] = K1.at<float>(1, 2);
    prob.K2[0] = K2.at<float>(0, 0); prob.K2[1] = K2.at<float>(1, 1); prob.K2[2] = K2.at<float>(0, 2); prob.K2[3] = K2.at<float>(1, 2);
    const cv::Mat T1 = pKF1->GetPose(), T2 = pKF2->GetPose();
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) { prob.Tcw1[r * 4 + c] = T1.at<float>(r, c); prob.Tcw2[r * 4 + c] = T2.at<float>(r, c); }
    const Eigen::Matrix3d R12 = g2oS12.rotation().toRotationMatrix();
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) prob.R[r * 3 + c] = (float)R12(r, c);
        prob.t[r] = (float)g2oS12.translation()[r];
    }
    prob.s = (float)g2oS12.scale();
    prob.th2 = th2;
    prob.fix_scale = bFixScale ? 1 : 0;

    const int N = (int)vpMatches1.size();
    const std::vector<MapPoint *> vpMapPoints1 = pKF1->GetMapPointMatches();
    std::vector<orbz_sim3_match_t> rows;
    std::vector<size_t> vnIndexEdge;
    rows.reserve(N); vnIndexEdge.reserve(N);
    for (int i = 0; i < N; i++) {   // :1104-1183
        if (!vpMatches1[i]) continue;
        MapPoint *pMP1 = vpMapPoints1[i];
        MapPoint *pMP2 = vpMatches1[i];
        const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
        if (!pMP1 || !pMP2) continue;
        if (pMP1->isBad() || pMP2->isBad() || i2 < 0) continue;
        orbz_sim3_match_t m;
        const cv::Mat P3D1w = pMP1->GetWorldPos(), P3D2w = pMP2->GetWorldPos();
        for (int k = 0; k < 3; k++) { m.w1[k] = P3D1w.at<float>(k); m.w2[k] = P3D2w.at<float>(k); }
        const cv::KeyPoint &kpUn1 = pKF1->mvKeysUn[i];
        const cv::KeyPoint &kpUn2 = pKF2->mvKeysUn[i2];
        m.u1 = kpUn1.pt.x; m.v1 = kpUn1.pt.y; m.u2 = kpUn2.pt.x; m.v2 = kpUn2.pt.y;
        m.inv_sigma2_1 = pKF1->mvInvLevelSigma2[kpUn1.octave];
        m.inv_sigma2_2 = pKF2->mvInvLevelSigma2[kpUn2.octave];
        rows.push_back(m);
        vnIndexEdge.push_back(i);
    }
    const int n = (int)rows.size();
    std::vector<uint8_t> dropped((size_t)n + 1, 0);
    float S12[16];
    int nIn = 0;
    orbz_sim3_info_t info;
    const int rc = orbz_optimize_sim3(rows.data(), n, &prob, S12, dropped.data(), &nIn, &info, device);
    if (rc != ORBX_OK) throw std::runtime_error(std::string("Optimizer::OptimizeSim3: ") + orbx_last_error());
    for (int k = 0; k < n; k++)
        if (dropped[k]) vpMatches1[vnIndexEdge[k]] = static_cast<MapPoint *>(NULL);
    if (info.rounds < 2) return 0;   // :1216-1217: returns before the vertex is read back
    g2oS12 = g2o::Sim3(Eigen::Quaterniond(info.q[3], info.q[0], info.q[1], info.q[2]), Eigen::Vector3d(info.t[0], info.t[1], info.t[2]), info.s);
    return nIn;
}

}  // namespace ORB_SLAM2
