// Optimizer.h — the members of ORB_SLAM2::Optimizer (include/Optimizer.h) executed on an MI355X through include/orbx.h:
// PoseOptimization (src/Optimizer.cc:239-451, orbo_pose_optimization), the pose-only optimisation Tracking runs between its matcher
// calls (src/Tracking.cc:918, :1041, :1083, :1585-1616); OptimizeSim3 (src/Optimizer.cc:1051-1246, orbz_optimize_sim3), the
// refinement of a loop candidate's Sim3 in LoopClosing::ComputeSim3 (src/LoopClosing.cc:336); LocalBundleAdjustment (:453-780,
// orbb_local_bundle_adjustment), the mapping thread's bundle adjustment (src/LocalMapping.cc:89), and BundleAdjustment /
// GlobalBundleAdjustemnt (:41-237) - orbb_bundle_adjustment for the map CreateInitialMapMonocular builds (src/Tracking.cc:700, nLoopKF
// == 0), orbb_global_bundle_adjustment for the loop closer's adjustment of the whole map (src/LoopClosing.cc:659, nLoopKF != 0).  The
// first two have ONE free vertex; the bundle adjustments marginalise the points, and the reduced system of a local window - a few tens
// of keyframes - is dense and small.  OptimizeEssentialGraph (:783-1049, orbg_optimize_essential_graph), the pose graph
// LoopClosing::CorrectLoop optimises (src/LoopClosing.cc:576), is here too: an earlier version of this comment filed it under "sparse,
// not part of this library", which was a statement about storage, not about the arithmetic - the block pattern is fixed, the host
// does the symbolic factorisation once per call and the device the 7x7 block arithmetic.  The bundle adjustment of a
// loop-closure-sized map has the same arithmetic as the local one and another reduced-system path: the Schur complement summed over
// the keyframe pairs that co-observe a point, the dense LDL^T blocked over the whole GPU.  No member of the optimiser is left to g2o.
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
    // The reference's signature and semantics (:453-780): the three lists of :455-504 with the mnBALocalForKF / mnBAFixedForKF marks, one
    // observation per (map point, keyframe that is not bad), the flat call, then under pMap->mMutexMapUpdate EraseMapPointMatch /
    // EraseObservation for every flagged observation, SetPose for the local keyframes, SetWorldPos and UpdateNormalAndDepth for the
    // local points.  *pbStopFlag is read where the reference reads it; set at :655 the call returns with nothing written.  The local
    // keyframe with mnId == 0 is fixed and keeps its pose byte for byte (the reference writes it back through its quaternion).
    // Throws std::runtime_error with orbx_last_error() when the library reports an error (no GPU among them).
    void static LocalBundleAdjustment(KeyFrame *pKF, bool *pbStopFlag, Map *pMap);
    // :49-237 and :41-46.  nLoopKF == 0: orbb_bundle_adjustment and the write-back into the map (SetPose, SetWorldPos,
    // UpdateNormalAndDepth).  nLoopKF != 0 (the loop closer's global adjustment): orbb_global_bundle_adjustment, and the results go
    // beside the map - mTcwGBA (4x4 CV_32F) and mnBAGlobalForKF = nLoopKF on every keyframe that is not bad, mPosGBA (3x1 CV_32F) and
    // mnBAGlobalForKF on every point of the problem; no SetPose, SetWorldPos or UpdateNormalAndDepth, and a bad point or one without
    // a usable observation (vbNotIncludedMP) is untouched.  *pbStopFlag is &mbStopGBA's: read before every iteration and after a
    // rejected trial.  Throws std::runtime_error with orbx_last_error() when the library reports an error.
    void static BundleAdjustment(const std::vector<KeyFrame *> &vpKFs, const std::vector<MapPoint *> &vpMP, int nIterations = 5,
                                 bool *pbStopFlag = NULL, const unsigned long nLoopKF = 0, const bool bRobust = true);
    void static GlobalBundleAdjustemnt(Map *pMap, int nIterations = 5, bool *pbStopFlag = NULL, const unsigned long nLoopKF = 0,
                                       const bool bRobust = true);
    // The reference's signature (:783-1049).  One vertex per keyframe of the map that is not bad (CorrectedSim3's entry or Sim3(Rcw, tcw,
    // 1) of its pose; NonCorrectedSim3's entry beside it; pLoopKF fixed), the four edge groups of :849-985 with every rule (minFeat =
    // 100, sInsertedEdges, the mnId comparisons, hasChild, sLoopEdges.count), one point per map point that is not bad (its vertex from
    // mnCorrectedReference or the reference keyframe), the flat call with 20 iterations, then under pMap->mMutexMapUpdate SetPose,
    // SetWorldPos and UpdateNormalAndDepth.  Differences, all stated: LoopConnections and every std::set of keyframes are walked in
    // ascending mnId (the reference walks them in pointer order, which only orders g2o's sums); a bad keyframe gets no vertex, no edge
    // and no write-back (the reference's write-back loop dereferences its missing vertex); a point whose reference keyframe has no
    // vertex is left alone; pMap->UpdateKeyFrame (the multi-agent server) stays the caller's.  Throws std::runtime_error with
    // orbx_last_error() when the library reports an error (no GPU among them).
    void static OptimizeEssentialGraph(Map *pMap, KeyFrame *pLoopKF, KeyFrame *pCurKF, const LoopClosing::KeyFrameAndPose &NonCorrectedSim3,
                                       const LoopClosing::KeyFrameAndPose &CorrectedSim3,
                                       const std::map<KeyFrame *, std::set<KeyFrame *> > &LoopConnections, const bool &bFixScale);
    static int device;   // GPU used (default: ORBX_DEVICE or 0)
};

}  // namespace ORB_SLAM2
#endif
