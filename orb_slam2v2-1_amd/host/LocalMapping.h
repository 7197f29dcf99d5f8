// LocalMapping.h — the data-parallel member of ORB_SLAM2::LocalMapping (include/LocalMapping.h) executed on an MI355X through
// include/orbx.h: CreateNewMapPoints (src/LocalMapping.cc:215-460), the only place a running map grows, with ComputeF12 and
// SkewSymmetricMatrix (:544-561, :706-711).  The loop over the covisible neighbours - SearchForTriangulation, then per match the
// parallax test, the triangulation or stereo unprojection and the five acceptance tests - is ONE call of orbl_create_new_map_points:
// the flags that keep a feature which received a point from neighbour i from being a query for neighbour i + 1 are updated on the
// device.  What the reference does with an accepted match (new MapPoint, observations, descriptor, normal and depth, the recent
// list) is host code and runs here afterwards, neighbour by neighbour in ascending idx1: the reference's order.
// KeyFrameCulling (:640-704) is ONE call of orbc_keyframe_culling over the observation table built from the local keyframes
// (Covisibility.h): the device returns the verdicts of the reference's sequential loop, and SetBadFlag runs here on each, in order.
// SearchInNeighbors' control flow, MapPointCulling and the queue are not part of this library; local bundle adjustment is
// Optimizer.h's, UpdateConnections and UpdateNormalAndDepth for many objects are Covisibility.h's.
#ifndef ORBX_LOCALMAPPING_H
#define ORBX_LOCALMAPPING_H
#include <functional>
#include <list>
#include "frame_shim.h"

namespace ORB_SLAM2 {

class LocalMapping {
public:
    LocalMapping(Map *pMap, const float bMonocular) : mpCurrentKeyFrame(NULL), mbMonocular(bMonocular != 0), mpMap(pMap) {}
    // Reads mpCurrentKeyFrame and its GetBestCovisibilityKeyFrames(10 / 20 when monocular): pose, calibration, mb, mbf, mfScaleFactor,
    // level tables, mvKeysUn, mvKeys, mvuRight, mvDepth, mDescriptors, mFeatVec, GetMapPoint.  Creates the map points and pushes them
    // to mlpRecentAddedMapPoints.  Before it applies neighbour i > 0 it asks CheckNewKeyFrames() and, on true, discards the rest
    // (:247-248).  Throws std::runtime_error with orbx_last_error() when the library reports an error (no GPU among them).
    void CreateNewMapPoints();
    // Reads mpCurrentKeyFrame->GetVectorCovisibleKeyFrames() and of each of them mnId, mbNotErase, mThDepth, mvDepth, mvKeysUn,
    // mvuRight and the map points with their observations; calls SetBadFlag() on the keyframes the reference's loop would (the shim's:
    // no spanning tree).  The walk order of a point's observations is mnId order, not pointer order; no result depends on it.
    // Throws std::runtime_error with orbx_last_error() when the library reports an error (no GPU among them).
    void KeyFrameCulling();
    cv::Mat ComputeF12(KeyFrame *&pKF1, KeyFrame *&pKF2);
    cv::Mat SkewSymmetricMatrix(const cv::Mat &v);
    bool CheckNewKeyFrames() { return mCheckNewKeyFrames ? mCheckNewKeyFrames() : false; }
    // the reference asks its queue of new keyframes (:96-100); here the caller says how
    void SetCheckNewKeyFrames(const std::function<bool()> &f) { mCheckNewKeyFrames = f; }

    KeyFrame *mpCurrentKeyFrame;
    bool mbMonocular;
    Map *mpMap;
    std::list<MapPoint *> mlpRecentAddedMapPoints;
    static int device;   // GPU used (default: ORBX_DEVICE or 0)

private:
    std::function<bool()> mCheckNewKeyFrames;
};

}  // namespace ORB_SLAM2
#endif
