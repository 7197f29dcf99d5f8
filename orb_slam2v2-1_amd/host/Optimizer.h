// Optimizer.h — ORB_SLAM2::Optimizer::PoseOptimization (include/Optimizer.h, src/Optimizer.cc:239-451) executed on an MI355X through
// include/orbx.h (orbo_pose_optimization): the pose-only optimisation Tracking runs between its matcher calls
// (src/Tracking.cc:918, :1041, :1083, :1585-1616).  The other members of the reference's Optimizer (bundle adjustment, Sim3,
// essential graph) are sparse problems of another shape and are not part of this library: keep the reference's own for them.
#ifndef ORBX_OPTIMIZER_H
#define ORBX_OPTIMIZER_H
#include "frame_shim.h"

namespace ORB_SLAM2 {

class Optimizer {
public:
    // Reads mvpMapPoints (GetWorldPos), mvKeysUn, mvuRight, mvInvLevelSigma2, fx fy cx cy mbf and mTcw; writes mvbOutlier of the entries
    // that hold a map point and the pose (SetPose); returns nInitialCorrespondences - nBad.  Fewer than 3 correspondences: 0, the
    // pose untouched.  Throws std::runtime_error with orbx_last_error() when the library reports an error (no GPU among them).
    int static PoseOptimization(Frame *pFrame);
    static int device;   // GPU used (default: ORBX_DEVICE or 0)
};

}  // namespace ORB_SLAM2
#endif
