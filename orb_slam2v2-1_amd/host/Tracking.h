// Tracking.h — Tracking::UpdateLocalMap and Tracking::SearchLocalPoints (reference: src/Tracking.cc:1288-1484) with the local map
// computed on an MI355X through include/orbx.h (orbt_*): LocalMapHIP keeps a snapshot of the map on the device, Tracking makes ONE
// call per frame and writes the members the reference writes.
//
// When to Rebuild: whenever LocalMapping or LoopClosing changed the map (keyframes or points added, erased or set bad, observations,
// covisibility lists or the spanning tree changed), under Map::mMutexMapUpdate, before the next UpdateLocalMap.  A point of the frame
// that the snapshot does not know (Tracking's own temporal points of UpdateLastFrame, which have no observations) votes for nothing
// and is in no keyframe: it is handled on the host.
//
// Stated differences from the reference: keyframes get their slots in ascending mnId, so the first-stage keyframes come in mnId order
// where the reference walks a std::map<KeyFrame*, int> in pointer order, and the reference keyframe among equal votes is the one with
// the smallest mnId; children are visited in ascending mnId where the reference walks a std::set<KeyFrame*>; the extension loop walks
// the first-stage entries by index (the reference's iterators are undefined once its reserve(3 * size) is exceeded).
// Kept quirks: a parent is appended without isBad() (:1466-1469), and the `break` after it (:1473) ends the whole extension loop.
// Map::SetReferenceMapPoints (:1343) stays the caller's.
#ifndef ORBX_TRACKING_H
#define ORBX_TRACKING_H
#include <map>
#include <vector>
#include "Covisibility.h"
#include "frame_shim.h"
#include "orbx.h"

namespace ORB_SLAM2 {

#ifndef ORBX_HAVE_ORBSLAM2
struct System { enum eSensor { MONOCULAR = 0, STEREO = 1, RGBD = 2 }; };   // include/System.h:61-65
#endif

// The resident snapshot: every keyframe and map point of the map, the graph, the points' views and descriptors
class LocalMapHIP {
public:
    LocalMapHIP();
    ~LocalMapHIP();
    // packs GetAllKeyFrames() / GetAllMapPoints() and uploads them.  Throws std::runtime_error with orbx_last_error() when the library
    // reports an error (no GPU among them)
    void Rebuild(Map *pMap);
    CovisTables T;                              // slot -> keyframe, point index -> map point
    std::map<MapPoint *, int32_t> index;        // map point -> point index
    orbt_localmap_t *handle;
    static int device;                          // GPU used (default: ORBX_DEVICE or 0)
private:
    LocalMapHIP(const LocalMapHIP &);
    LocalMapHIP &operator=(const LocalMapHIP &);
};

class Tracking {
public:
    Tracking() : mpReferenceKF(NULL), mpMap(NULL), mSensor(System::MONOCULAR), mnLastRelocFrameId(0), mnMatchesLocal(0), mnToMatch(0) {}
    // src/Tracking.cc:1340-1484 without :1343: NULLs the bad slots of mCurrentFrame.mvpMapPoints, writes mvpLocalKeyFrames and
    // mvpLocalMapPoints, the mnTrackReferenceForFrame marks of both, mpReferenceKF and mCurrentFrame.mpReferenceKF.  Throws as Rebuild
    void UpdateLocalMap();
    // src/Tracking.cc:1288-1338: the first loop on the host, then the arrays UpdateLocalMap received go to orbm_search_local_points
    // unchanged; the results are applied as SearchLocalPointsHIP (ORBmatcher.h) applies them.  th is 1 / 3 / 5 (:1330-1335)
    void SearchLocalPoints();
    Frame mCurrentFrame;
    std::vector<KeyFrame *> mvpLocalKeyFrames;
    std::vector<MapPoint *> mvpLocalMapPoints;
    KeyFrame *mpReferenceKF;
    Map *mpMap;
    int mSensor;
    unsigned int mnLastRelocFrameId;
    LocalMapHIP mLocalMap;
    orbt_local_info_t mLocalInfo;               // of the last UpdateLocalMap
    int mnMatchesLocal, mnToMatch;              // of the last SearchLocalPoints: the matcher's return value and nToMatch (:1309-1325)
private:
    // what the last UpdateLocalMap received for SearchLocalPoints
    std::vector<orbm_worldpoint_t> mLocalPts;
    std::vector<uint8_t> mLocalDesc;
    std::vector<int32_t> mHolder, mExtObs, mLkf, mLpts;
};

}  // namespace ORB_SLAM2
#endif
