// LoopClosing.h — the two map-sized loops of ORB_SLAM2::LoopClosing (reference: src/LoopClosing.cc:444-525 and :685-746) executed on
// an MI355X through include/orbx.h (orbr_*): the tables are built from the objects, uploaded once per call, and the results are
// written back to the members the reference writes.  The control flow around them - stop requests, the mutexes, the mnFullBAIdx
// test, the fusion half of CorrectLoop - stays the caller's.
//
// Stated differences from the reference: keyframes get their slots in ascending mnId, so CorrectedSim3 is walked in mnId order where
// the reference walks a std::map<KeyFrame*, g2o::Sim3> in pointer order (a point seen by several connected keyframes is corrected by
// the one with the smallest mnId), and a normal's sum runs in mnId order, as Covisibility.h states.  A map point whose reference
// keyframe is not among its observers keeps its normal and distances (the reference's observations[pRefKF] inserts index 0 there).
// A point whose reference keyframe is NULL, or is marked but was never reached from the origins (its mTcwBefGBA is empty), keeps its
// position in UpdateMapAfterGlobalBA, where the reference dereferences it.
#ifndef ORBX_LOOPCLOSING_H
#define ORBX_LOOPCLOSING_H
#include <functional>
#include <map>
#include <vector>
#include "g2o_shim.h"   // g2o::Sim3; it includes this header back where the reference's Converter.h users expect LoopClosing
#include "frame_shim.h"

namespace ORB_SLAM2 {

class LoopClosing {
public:
    typedef std::map<KeyFrame *, g2o::Sim3, std::less<KeyFrame *> > KeyFrameAndPose;   // include/LoopClosing.h:50-51, without Eigen's allocator
    LoopClosing() : mpCurrentKF(NULL), mpMap(NULL) {}
    // src/LoopClosing.cc:444-525: mvpCurrentConnectedKFs = the current keyframe's covisibles and itself; fills the two maps
    // OptimizeEssentialGraph takes; SetWorldPos, mnCorrectedByKF, mnCorrectedReference, mNormalVector / mfMaxDistance / mfMinDistance of
    // every corrected point; SetPose of every connected keyframe; then UpdateConnections of the connected keyframes (:524) with ONE
    // more device call on the same table.  Throws std::runtime_error with orbx_last_error() when the library reports an error
    void CorrectLoopPoses(KeyFrameAndPose &CorrectedSim3, KeyFrameAndPose &NonCorrectedSim3);
    // src/LoopClosing.cc:685-746 after Optimizer::GlobalBundleAdjustemnt(.., nLoopKF, ..): mTcwGBA and mnBAGlobalForKF of the keyframes
    // the spanning tree reaches outside the global BA, mTcwBefGBA and SetPose of every keyframe reached from mpMap->mvpKeyFrameOrigins,
    // SetWorldPos of every point that took mPosGBA or moved with its reference keyframe.  Throws as above
    void UpdateMapAfterGlobalBA(unsigned long nLoopKF);
    KeyFrame *mpCurrentKF;
    g2o::Sim3 mg2oScw;
    std::vector<KeyFrame *> mvpCurrentConnectedKFs;
    Map *mpMap;
    static int device;   // GPU used (default: ORBX_DEVICE or 0)
};

}  // namespace ORB_SLAM2
#endif
