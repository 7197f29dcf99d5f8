// frame_shim.h — the members of ORB_SLAM2::Frame / MapPoint that the hot matchers read or
// write (reference: include/Frame.h:100-188, include/MapPoint.h), so that ORBmatcher.cc
// compiles and is testable here without the rest of ORB-SLAM2.  In the reference tree, define
// ORBX_HAVE_ORBSLAM2 and the real "Frame.h" / "MapPoint.h" are used instead: the sources only
// touch members that exist there under the same names.
#pragma once
#ifdef ORBX_HAVE_ORBSLAM2
#include "Frame.h"
#include "MapPoint.h"
#else
#include <algorithm>
#include <climits>
#include <cmath>
#include <map>
#include <mutex>
#include <set>
#include <vector>
#include "cv_shim.h"
#include "ORBextractor.h"
#include "ORBVocabulary.h"

namespace ORB_SLAM2 {

class Frame;
class KeyFrame;
class MapPoint;

class Map {   // include/Map.h: what LocalMapping::CreateNewMapPoints and Optimizer::LocalBundleAdjustment / GlobalBundleAdjustemnt touch
public:
    void AddKeyFrame(KeyFrame *pKF) { mvpKeyFrames.push_back(pKF); }   // src/Map.cc:33-40 (a set there)
    std::vector<KeyFrame *> GetAllKeyFrames() { return mvpKeyFrames; }
    std::vector<KeyFrame *> mvpKeyFrames;
    std::mutex mMutexMapUpdate;
    void AddMapPoint(MapPoint *pMP) { mvpMapPoints.push_back(pMP); }   // src/Map.cc:42-46 (a set there; insertion order is kept here for the tests)
    std::vector<MapPoint *> GetAllMapPoints() { return mvpMapPoints; }
    std::vector<MapPoint *> mvpMapPoints;
    inline long unsigned int GetMaxKFid();   // src/Map.cc:106-110 (kept as a member there; the largest mnId in the map here)
    std::vector<KeyFrame *> mvpKeyFrameOrigins;   // include/Map.h: where LoopClosing::RunGlobalBundleAdjustment starts its walk of the spanning tree
};

class MapPoint {
public:
    // src/MapPoint.cc:31-50, without the ids: the position, a zero normal, the reference keyframe
    inline MapPoint(const cv::Mat &Pos, KeyFrame *pRefKF, Map *pMap);
    // host code after src/MapPoint.cc:252-317 and :340-383, on the shim's members
    inline void ComputeDistinctiveDescriptors();
    inline void UpdateNormalAndDepth();
    KeyFrame *mpRefKF = NULL;
    Map *mpMap = NULL;
    MapPoint() : mbTrackInView(false), mnTrackScaleLevel(0), mTrackViewCos(1.f), mTrackProjX(0), mTrackProjY(0),
                 mTrackProjXR(0), mbBad(false), nObs(0) { mWorldPos = cv::Mat::zeros(3, 1, CV_32F); }
    // tracking variables set by Frame::isInFrustum (src/Frame.cc:284-340)
    bool mbTrackInView;
    int mnTrackScaleLevel;
    float mTrackViewCos, mTrackProjX, mTrackProjY, mTrackProjXR;
    bool isBad() { return mbBad; }
    int Observations() { return nObs; }
    cv::Mat GetDescriptor() { return mDescriptor.clone(); }  // src/MapPoint.cc:319-323
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    // scale-invariance distances (src/MapPoint.cc:385-395) and level prediction (:414-429)
    float GetMinDistanceInvariance() { return 0.8f * mfMinDistance; }
    float GetMaxDistanceInvariance() { return 1.2f * mfMaxDistance; }
    inline int PredictScale(const float &currentDist, Frame *pF);
    inline int PredictScale(const float &currentDist, KeyFrame *pKF);   // src/MapPoint.cc:397-412
    cv::Mat GetNormal() { return mNormalVector.clone(); }
    // observation graph, reduced to what ORBmatcher::Fuse / SearchBySim3 touch
    bool IsInKeyFrame(KeyFrame *pKF) { return mObservations.count(pKF) != 0; }            // src/MapPoint.cc
    int GetIndexInKeyFrame(KeyFrame *pKF) { return mObservations.count(pKF) ? (int)mObservations[pKF] : -1; }
    inline void AddObservation(KeyFrame *pKF, size_t idx);                                // src/MapPoint.cc:108-119
    inline void EraseObservation(KeyFrame *pKF);                                          // src/MapPoint.cc:121-147
    inline void SetBadFlag();                                                             // src/MapPoint.cc:161-180, without the Map erase
    void SetWorldPos(const cv::Mat &Pos) { mWorldPos = Pos.clone(); }                     // src/MapPoint.cc:83-88
    long unsigned int mnId = 0, mnBALocalForKF = 0;   // include/MapPoint.h: read and written by Optimizer::LocalBundleAdjustment
    long unsigned int mnCorrectedByKF = 0, mnCorrectedReference = 0;   // include/MapPoint.h: set by LoopClosing::CorrectLoop, read by Optimizer::OptimizeEssentialGraph
    cv::Mat mPosGBA;                      // include/MapPoint.h: written by Optimizer::BundleAdjustment with nLoopKF != 0 (3x1 CV_32F), read by
    long unsigned int mnBAGlobalForKF = 0;   // LoopClosing::RunGlobalBundleAdjustment
    KeyFrame *GetReferenceKeyFrame() { return mpRefKF; }   // src/MapPoint.cc:96-100
    inline void Replace(MapPoint *pMP);                                                   // src/MapPoint.cc:187-225
    std::map<KeyFrame *, size_t> GetObservations() { return mObservations; }
    void SetDescriptor(const cv::Mat &d) { mDescriptor = d.clone(); }   // the store at src/MapPoint.cc:313-316 (test shim only)
    bool mbBad;
    int nObs;
    long unsigned int mnLastFrameSeen = 0;   // include/MapPoint.h
    long unsigned int mnTrackReferenceForFrame = 0;   // include/MapPoint.h: the mark of Tracking::UpdateLocalPoints
    int mnVisible = 1;
    void IncreaseVisible(int n = 1) { mnVisible += n; }
    float mfMinDistance = 0.f, mfMaxDistance = 0.f;
    cv::Mat mDescriptor, mWorldPos;
    cv::Mat mNormalVector = cv::Mat::zeros(3, 1, CV_32F);
    std::map<KeyFrame *, size_t> mObservations;
};

class Frame {
public:
    Frame() : mpORBextractorLeft(nullptr), mpORBextractorRight(nullptr), mbf(0), mb(0), N(0) {}
    long unsigned int mnId = 0;
    // BoW (include/Frame.h:133-138, src/Frame.cc:410-417)
    ORBVocabulary *mpORBvocabulary = nullptr;
    DBoW2::BowVector mBowVec;
    DBoW2::FeatureVector mFeatVec;
    void ComputeBoW() {
        if (mBowVec.empty()) {
            std::vector<cv::Mat> vCurrentDesc;   // Converter::toDescriptorVector
            for (int j = 0; j < mDescriptors.rows; j++) vCurrentDesc.push_back(mDescriptors.row(j));
            mpORBvocabulary->transform(vCurrentDesc, mBowVec, mFeatVec, 4);
        }
    }
    ORBextractor *mpORBextractorLeft, *mpORBextractorRight;
    static float fx, fy, cx, cy;
    cv::Mat mK, mDistCoef;   // calibration (include/Frame.h): 3x3 and 4x1 / 5x1 CV_32F
    float mbf, mb;
    int N;
    std::vector<cv::KeyPoint> mvKeys, mvKeysRight, mvKeysUn;
    std::vector<float> mvuRight, mvDepth;
    cv::Mat mDescriptors, mDescriptorsRight;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    KeyFrame *mpReferenceKF = nullptr;   // include/Frame.h: set by Tracking::UpdateLocalKeyFrames
    static float mfGridElementWidthInv, mfGridElementHeightInv;
    cv::Mat mTcw;
    void SetPose(cv::Mat Tcw) { mTcw = Tcw.clone(); }   // src/Frame.cc:262-266, without the derived Rcw / tcw / Ow the matchers do not read
    std::vector<float> mvScaleFactors, mvInvScaleFactors, mvInvLevelSigma2;
    std::vector<float> mvLevelSigma2;   // include/Frame.h: read by PnPsolver
    static float mnMinX, mnMaxX, mnMinY, mnMaxY;
    int mnScaleLevels = 0;          // src/Frame.cc:69
    float mfScaleFactor = 0.f, mfLogScaleFactor = 0.f;  // :70-71
};

inline int MapPoint::PredictScale(const float &currentDist, Frame *pF) {
    using namespace std;
    float ratio = mfMaxDistance / currentDist;
    int nScale = ceil(log(ratio) / pF->mfLogScaleFactor);
    if (nScale < 0) nScale = 0;
    else if (nScale >= pF->mnScaleLevels) nScale = pF->mnScaleLevels - 1;
    return nScale;
}

class KeyFrame {   // include/KeyFrame.h: the members the projection matchers read or write
public:
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }  // src/KeyFrame.cc
    std::set<MapPoint *> GetMapPoints() {
        std::set<MapPoint *> s;
        for (size_t i = 0; i < mvpMapPoints.size(); i++)
            if (mvpMapPoints[i] && !mvpMapPoints[i]->isBad()) s.insert(mvpMapPoints[i]);
        return s;
    }
    bool isBad() { return mbBad; }
    bool mbBad = false;
    ORBVocabulary *mpORBvocabulary = nullptr;   // src/KeyFrame.cc:59-68
    DBoW2::BowVector mBowVec;
    DBoW2::FeatureVector mFeatVec;
    void ComputeBoW() {
        if (mBowVec.empty() || mFeatVec.empty()) {
            std::vector<cv::Mat> vCurrentDesc;
            for (int j = 0; j < mDescriptors.rows; j++) vCurrentDesc.push_back(mDescriptors.row(j));
            mpORBvocabulary->transform(vCurrentDesc, mBowVec, mFeatVec, 4);
        }
    }
    MapPoint *GetMapPoint(const size_t &idx) { return mvpMapPoints[idx]; }
    void AddMapPoint(MapPoint *pMP, const size_t &idx) { mvpMapPoints[idx] = pMP; }
    void ReplaceMapPointMatch(const size_t &idx, MapPoint *pMP) { mvpMapPoints[idx] = pMP; }
    void EraseMapPointMatch(const size_t &idx) { mvpMapPoints[idx] = static_cast<MapPoint *>(NULL); }
    void EraseMapPointMatch(MapPoint *pMP) {   // src/KeyFrame.cc:223-228
        int idx = pMP->GetIndexInKeyFrame(this);
        if (idx >= 0) mvpMapPoints[idx] = static_cast<MapPoint *>(NULL);
    }
    long unsigned int mnBALocalForKF = 0, mnBAFixedForKF = 0;   // include/KeyFrame.h: the marks of Optimizer::LocalBundleAdjustment
    cv::Mat mTcwGBA, mTcwBefGBA;          // include/KeyFrame.h: mTcwGBA (4x4 CV_32F) and the mark are written by Optimizer::BundleAdjustment with
    long unsigned int mnBAGlobalForKF = 0;   // nLoopKF != 0; mTcwBefGBA is LoopClosing::RunGlobalBundleAdjustment's own
    // the spanning tree, the loop edges and the covisibility weights, as far as Optimizer::OptimizeEssentialGraph reads them
    // (src/KeyFrame.cc:137-146, :326-359, :404-448)
    KeyFrame *mpParent = NULL;
    std::set<KeyFrame *> mspChildrens, mspLoopEdges;
    std::map<KeyFrame *, int> mConnectedKeyFrameWeights;
    KeyFrame *GetParent() { return mpParent; }
    std::set<KeyFrame *> GetChilds() { return mspChildrens; }   // src/KeyFrame.cc:398-402
    long unsigned int mnTrackReferenceForFrame = 0;   // include/KeyFrame.h: the mark of Tracking::UpdateLocalKeyFrames
    bool hasChild(KeyFrame *pKF) { return mspChildrens.count(pKF) != 0; }
    std::set<KeyFrame *> GetLoopEdges() { return mspLoopEdges; }
    int GetWeight(KeyFrame *pKF) { return mConnectedKeyFrameWeights.count(pKF) ? mConnectedKeyFrameWeights[pKF] : 0; }
    std::vector<KeyFrame *> GetCovisiblesByWeight(const int &w) {   // the head of the ordered list whose weight is at least w
        std::vector<KeyFrame *> v;
        for (size_t i = 0; i < mvpOrderedConnectedKeyFrames.size(); i++) {
            if (GetWeight(mvpOrderedConnectedKeyFrames[i]) < w) break;
            v.push_back(mvpOrderedConnectedKeyFrames[i]);
        }
        return v;
    }
    std::vector<KeyFrame *> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }   // src/KeyFrame.cc:310-314
    cv::Mat GetPose() { return Tcw.clone(); }
    cv::Mat GetRotation() {
        cv::Mat R(3, 3, CV_32F);
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) R.at<float>(r, c) = Tcw.at<float>(r, c);
        return R;
    }
    cv::Mat GetTranslation() {
        cv::Mat t(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) t.at<float>(r) = Tcw.at<float>(r, 3);
        return t;
    }
    cv::Mat GetCameraCenter() { return Ow.clone(); }
    void SetPose(const cv::Mat &Tcw_) {   // src/KeyFrame.cc:70-84: Ow = -Rwc*tcw (gemm, alpha = -1)
        Tcw = Tcw_.clone();
        Ow = cv::Mat(3, 1, CV_32F);
        for (int i = 0; i < 3; i++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += (double)Tcw.at<float>(k, i) * (double)Tcw.at<float>(k, 3);
            Ow.at<float>(i) = (float)(s * -1.0);
        }
    }
    bool IsInImage(const float &x, const float &y) const { return (x >= mnMinX && x < mnMaxX && y >= mnMinY && y < mnMaxY); }
    float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
    float invfx = 0, invfy = 0, mb = 0, mfScaleFactor = 0;   // include/KeyFrame.h: read by LocalMapping::CreateNewMapPoints
    long unsigned int mnId = 0;
    cv::Mat mK;   // include/KeyFrame.h: the 3x3 CV_32F calibration, read by Optimizer::OptimizeSim3
    int N = 0;
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;   // mvKeys: the raw keypoints, which UnprojectStereo reads
    std::vector<float> mvuRight, mvDepth;
    // the covisibility graph reduced to its result: the ordered list (src/KeyFrame.cc:316-324 returns its first N entries)
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;
    std::vector<int> mvOrderedWeights;   // include/KeyFrame.h: the weights of mvpOrderedConnectedKeyFrames (src/KeyFrame.cc:370)
    // what LocalMapping::KeyFrameCulling reads and sets (include/KeyFrame.h)
    bool mbNotErase = false, mbToBeErased = false;
    float mThDepth = 0.f;
    // src/KeyFrame.cc:454-472 plus mbBad = true (:540): the early returns, the neighbours forget this keyframe (EraseConnection, :554-569,
    // whose re-sort of a consistent list is the list without the entry), then every map point does.  No spanning tree (:480-539), no
    // map and no keyframe database (:544-545): the shim has none of them to repair
    void SetBadFlag() {
        if (mnId == 0) return;
        else if (mbNotErase) { mbToBeErased = true; return; }
        for (std::map<KeyFrame *, int>::iterator mit = mConnectedKeyFrameWeights.begin(), mend = mConnectedKeyFrameWeights.end(); mit != mend; mit++) {
            KeyFrame *o = mit->first;
            if (!o->mConnectedKeyFrameWeights.erase(this)) continue;
            for (size_t i = 0; i < o->mvpOrderedConnectedKeyFrames.size(); i++)
                if (o->mvpOrderedConnectedKeyFrames[i] == this) {
                    o->mvpOrderedConnectedKeyFrames.erase(o->mvpOrderedConnectedKeyFrames.begin() + i);
                    if (i < o->mvOrderedWeights.size()) o->mvOrderedWeights.erase(o->mvOrderedWeights.begin() + i);
                    break;
                }
        }
        for (size_t i = 0; i < mvpMapPoints.size(); i++)
            if (mvpMapPoints[i]) mvpMapPoints[i]->EraseObservation(this);
        mbBad = true;
    }
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(const int &n) {
        if ((int)mvpOrderedConnectedKeyFrames.size() < n) return mvpOrderedConnectedKeyFrames;
        return std::vector<KeyFrame *>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + n);
    }
    // src/KeyFrame.cc:636-666: z = Rcw.row(2).dot(x3Dw) + zcw (the dot product a double), the sorted depths' entry (size-1)/q.  No map point:
    // the reference indexes an empty vector; 0 here
    float ComputeSceneMedianDepth(const int q) {
        std::vector<float> vDepths;
        for (int i = 0; i < N; i++)
            if (mvpMapPoints[i]) {
                cv::Mat x3Dw = mvpMapPoints[i]->GetWorldPos();
                double s = 0;
                for (int k = 0; k < 3; k++) s += (double)Tcw.at<float>(2, k) * (double)x3Dw.at<float>(k);
                vDepths.push_back((float)(s + (double)Tcw.at<float>(2, 3)));
            }
        if (vDepths.empty()) return 0.f;
        std::sort(vDepths.begin(), vDepths.end());
        return vDepths[(vDepths.size() - 1) / q];
    }
    cv::Mat mDescriptors;
    int mnScaleLevels = 0;
    float mfLogScaleFactor = 0.f;
    std::vector<float> mvScaleFactors, mvInvLevelSigma2, mvLevelSigma2;
    int mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0;   // ints: include/KeyFrame.h:199-202
    float mfGridElementWidthInv = 0.f, mfGridElementHeightInv = 0.f;
    std::vector<MapPoint *> mvpMapPoints;
    cv::Mat Tcw = cv::Mat::eye(4, 4, CV_32F), Ow = cv::Mat::zeros(3, 1, CV_32F);
};

inline long unsigned int Map::GetMaxKFid() {
    long unsigned int m = 0;
    for (size_t i = 0; i < mvpKeyFrames.size(); i++) m = std::max(m, mvpKeyFrames[i]->mnId);
    return m;
}
inline int MapPoint::PredictScale(const float &currentDist, KeyFrame *pKF) {
    using namespace std;
    float ratio = mfMaxDistance / currentDist;
    int nScale = ceil(log(ratio) / pKF->mfLogScaleFactor);
    if (nScale < 0) nScale = 0;
    else if (nScale >= pKF->mnScaleLevels) nScale = pKF->mnScaleLevels - 1;
    return nScale;
}
inline void MapPoint::AddObservation(KeyFrame *pKF, size_t idx) {
    if (mObservations.count(pKF)) return;
    mObservations[pKF] = idx;
    if (pKF->mvuRight[idx] >= 0) nObs += 2; else nObs++;
}
inline void MapPoint::EraseObservation(KeyFrame *pKF) {
    bool bBad = false;
    if (mObservations.count(pKF)) {
        int idx = (int)mObservations[pKF];
        if (pKF->mvuRight[idx] >= 0) nObs -= 2; else nObs--;
        mObservations.erase(pKF);
        if (mpRefKF == pKF) mpRefKF = mObservations.empty() ? NULL : mObservations.begin()->first;
        if (nObs <= 2) bBad = true;   // if only 2 observations or less, discard point
    }
    if (bBad) SetBadFlag();
}
inline void MapPoint::SetBadFlag() {
    std::map<KeyFrame *, size_t> obs = mObservations;
    mbBad = true;
    mObservations.clear();
    for (std::map<KeyFrame *, size_t>::iterator mit = obs.begin(), mend = obs.end(); mit != mend; mit++) mit->first->EraseMapPointMatch(mit->second);
}
inline MapPoint::MapPoint(const cv::Mat &Pos, KeyFrame *pRefKF, Map *pMap) : MapPoint() {
    mWorldPos = Pos.clone();
    mpRefKF = pRefKF;
    mpMap = pMap;
}
inline void MapPoint::ComputeDistinctiveDescriptors() {
    if (mbBad || mObservations.empty()) return;
    std::vector<cv::Mat> vDescriptors;
    for (std::map<KeyFrame *, size_t>::iterator mit = mObservations.begin(), mend = mObservations.end(); mit != mend; mit++)
        if (!mit->first->isBad()) vDescriptors.push_back(mit->first->mDescriptors.row((int)mit->second));
    if (vDescriptors.empty()) return;
    const size_t n = vDescriptors.size();
    std::vector<int> D(n * n, 0);
    for (size_t i = 0; i < n; i++)
        for (size_t j = i + 1; j < n; j++) {
            int d = 0;
            const unsigned char *a = vDescriptors[i].ptr(0), *b = vDescriptors[j].ptr(0);
            for (int k = 0; k < 32; k++) d += __builtin_popcount((unsigned)(a[k] ^ b[k]));
            D[i * n + j] = D[j * n + i] = d;
        }
    int BestMedian = INT_MAX, BestIdx = 0;   // the descriptor with least median distance to the rest
    for (size_t i = 0; i < n; i++) {
        std::vector<int> vDists(D.begin() + i * n, D.begin() + (i + 1) * n);
        std::sort(vDists.begin(), vDists.end());
        const int median = vDists[(size_t)(0.5 * (n - 1))];
        if (median < BestMedian) { BestMedian = median; BestIdx = (int)i; }
    }
    mDescriptor = vDescriptors[BestIdx].clone();
}
inline void MapPoint::UpdateNormalAndDepth() {
    if (mbBad || mObservations.empty() || !mpRefKF) return;
    float normal[3] = {0.f, 0.f, 0.f};
    int n = 0;
    for (std::map<KeyFrame *, size_t>::iterator mit = mObservations.begin(), mend = mObservations.end(); mit != mend; mit++) {
        cv::Mat Owi = mit->first->GetCameraCenter();
        float normali[3];
        double s = 0;
        for (int k = 0; k < 3; k++) { normali[k] = mWorldPos.at<float>(k) - Owi.at<float>(k); s += (double)normali[k] * (double)normali[k]; }
        const float inv = (float)(1.0 / std::sqrt(s));   // normal + normali/cv::norm(normali): a scaleAdd with a float factor
        for (int k = 0; k < 3; k++) normal[k] = normali[k] * inv + normal[k];
        n++;
    }
    cv::Mat Or = mpRefKF->GetCameraCenter();
    double s = 0;
    for (int k = 0; k < 3; k++) { const float d = mWorldPos.at<float>(k) - Or.at<float>(k); s += (double)d * (double)d; }
    const float dist = (float)std::sqrt(s);
    const int level = mpRefKF->mvKeysUn[mObservations[mpRefKF]].octave;
    mfMaxDistance = dist * mpRefKF->mvScaleFactors[level];
    mfMinDistance = mfMaxDistance / mpRefKF->mvScaleFactors[mpRefKF->mnScaleLevels - 1];
    for (int k = 0; k < 3; k++) mNormalVector.at<float>(k) = (float)((double)normal[k] * (1.0 / n));
}
inline void MapPoint::Replace(MapPoint *pMP) {   // without the found/visible counters, descriptor refresh and Map erase
    if (pMP == this) return;
    std::map<KeyFrame *, size_t> obs = mObservations;
    mObservations.clear();
    mbBad = true;
    for (std::map<KeyFrame *, size_t>::iterator mit = obs.begin(), mend = obs.end(); mit != mend; mit++) {
        KeyFrame *pKF = mit->first;
        if (!pMP->IsInKeyFrame(pKF)) { pKF->ReplaceMapPointMatch(mit->second, pMP); pMP->AddObservation(pKF, mit->second); }
        else pKF->EraseMapPointMatch(mit->second);
    }
}

}  // namespace ORB_SLAM2
#endif
