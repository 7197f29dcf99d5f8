// Covisibility.h — KeyFrame::UpdateConnections (src/KeyFrame.cc:290-380) and MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:340-383)
// for MANY objects in one call each, executed on an MI355X through include/orbx.h (orbc_*): the observation table is built from the
// objects, uploaded once, and the results are written back to the members the reference writes.  LocalMapping::KeyFrameCulling
// (LocalMapping.h) builds its table with the same CovisTables.
//
// Stated differences from the reference: keyframes get their slots in ascending mnId, so wherever the reference's order is the
// pointer order of a std::map<KeyFrame*, ...> (the tie-break of equal weights, the first keyframe that reaches the maximum, the order
// of a normal's sum) it is mnId order here, as Optimizer.h states for its sets.  UpdateConnectionsHIP does not touch the spanning
// tree: mbFirstConnection / mpParent (:372-377) stay the caller's.  A map point whose reference keyframe is not among its observers
// is left untouched by UpdateNormalAndDepthHIP (the reference's observations[pRefKF] inserts index 0 there, :373).
#ifndef ORBX_COVISIBILITY_H
#define ORBX_COVISIBILITY_H
#include <map>
#include <vector>
#include "frame_shim.h"
#include "orbx.h"

namespace ORB_SLAM2 {

// The table of include/orbx.h built from objects.  Keyframes: the queries, every observer of a listed point and every reference
// keyframe, in ascending mnId.  Points: the ones given, then every point a query's feature names, each once.
struct CovisTables {
    std::vector<KeyFrame *> kfs;                  // slot -> keyframe
    std::map<KeyFrame *, int32_t> slot;
    std::vector<MapPoint *> pts;                  // point index -> map point
    std::vector<orbc_keyframe_t> kf;
    std::vector<orbc_point_t> pt;
    std::vector<int32_t> obs_off, query_kf, feat_off;
    std::vector<orbc_observation_t> obs;
    std::vector<orbc_feature_t> feat;
    std::vector<float> sf;
    orbc_table_t table;
    orbc_queries_t queries;
    void Build(const std::vector<KeyFrame *> &vpQueries, const std::vector<MapPoint *> &vpPoints);
};

// UpdateConnections of every keyframe of the list, in the list's order, with ONE device call: writes mConnectedKeyFrameWeights,
// mvpOrderedConnectedKeyFrames and mvOrderedWeights, and the other side's weight and ordered lists as AddConnection does (:123-137).
// A keyframe none of whose points is seen elsewhere is left as it is (:324-325).  Throws std::runtime_error with orbx_last_error()
// when the library reports an error (no GPU among them).
void UpdateConnectionsHIP(const std::vector<KeyFrame *> &vpKFs);
// ... on a table the caller built with T.Build(vpKFs, ..) (LoopClosing::CorrectLoopPoses: positions do not enter the connections)
void UpdateConnectionsHIP(CovisTables &T, const std::vector<KeyFrame *> &vpKFs);
// UpdateNormalAndDepth of every point of the list with ONE device call: writes mNormalVector, mfMaxDistance and mfMinDistance of
// the points the reference's early return (:349, :359) lets through.  Throws as above.
void UpdateNormalAndDepthHIP(const std::vector<MapPoint *> &vpMPs);

struct Covisibility { static int device; };   // GPU used (default: ORBX_DEVICE or 0)

}  // namespace ORB_SLAM2
#endif
