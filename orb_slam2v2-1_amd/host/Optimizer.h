// Optimizer.h — the two DENSE members of ORB_SLAM2::Optimizer (include/Optimizer.h) executed on an MI355X through include/orbx.h:
// PoseOptimization (src/Optimizer.cc:239-451, orbo_pose_optimization), the pose-only optimisation Tracking runs between its matcher
// calls (src/Tracking.cc:918, :1041, :1083, :1585-1616), and OptimizeSim3 (src/Optimizer.cc:1051-1246, orbz_optimize_sim3), the
// refinement of a loop candidate's Sim3 in LoopClosing::ComputeSim3 (src/LoopClosing.cc:336).  Both have ONE free vertex and fixed
// map points - a 6x6 and a 7x7 normal matrix - and a dense solver in the reference too.  BundleAdjustment, LocalBundleAdjustment and
// OptimizeEssentialGraph are sparse nonlinear least squares over many vertices, another shape of problem, and are not part of this
// library: keep the reference's own (g2o) for them.
#ifndef ORBX_OPTIMIZER_H
#define ORBX_OPTIMIZER_H
#include "frame_shim.h"
#include "g2o_shim.h"

namespace ORB_SLAM2 {

class Optimizer {
public:
    // Reads mvpMapPoints (GetWorldPos), mvKeysUn, mvuRight, mvInvLevelSigma2, fx fy cx cy mbf and mTcw; writes mvbOutlier of the entries
    // that hold a map point and the pose (SetPose); returns nInitialCorrespondences - nBad.  Fewer than 3 correspondences: 0, the
    // pose untouched.  Throws std::runtime_error with orbx_last_error() when the library reports an error (no GPU among them).
    int static PoseOptimization(Frame *pFrame);
    // The reference's signature and semantics.  A match i enters when vpMatches1[i], pKF1's map point i and their isBad() allow it and
    // vpMatches1[i] is observed in pKF2 (:1104-1141); reads GetWorldPos of both points, mvKeysUn / mvInvLevelSigma2 / mK and the pose
    // of both keyframes.  Nulls the entries of vpMatches1 dropped in either round; returns the inlier count of the second round and
    // writes g2oS12 from the kernel's double estimate - or returns 0 with the first round's entries nulled and g2oS12 UNTOUCHED when
    // fewer than 10 matches survive the first round (:1216-1217).  g2oS12 enters through the C ABI's float R, t, s, which is what
    // LoopClosing builds it from (:330-335); t and s of such a Sim3 pass unchanged, its rotation as (float)toRotationMatrix().
    // Throws std::runtime_error with orbx_last_error() when the library reports an error (no GPU among them).
    static int OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches1, g2o::Sim3 &g2oS12, const float th2,
                            const bool bFixScale);
    static int device;   // GPU used (default: ORBX_DEVICE or 0)
};

}  // namespace ORB_SLAM2
#endif
