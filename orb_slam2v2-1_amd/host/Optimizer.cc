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

}  // namespace ORB_SLAM2
