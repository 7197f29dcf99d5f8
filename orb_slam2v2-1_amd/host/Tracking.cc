// Tracking.cc — the local map calls of include/orbx.h over the shim's objects (see Tracking.h).
#include "Tracking.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include "ORBmatcher.h"

namespace ORB_SLAM2 {

int LocalMapHIP::device = std::getenv("ORBX_DEVICE") ? std::atoi(std::getenv("ORBX_DEVICE")) : 0;

namespace {
bool by_id(KeyFrame *a, KeyFrame *b) { return a->mnId != b->mnId ? a->mnId < b->mnId : a < b; }
void raise(const char *what) { throw std::runtime_error(std::string(what) + ": " + orbx_last_error()); }
}  // namespace

LocalMapHIP::LocalMapHIP() : handle(NULL) {}
LocalMapHIP::~LocalMapHIP() { orbt_localmap_destroy(handle); }

void LocalMapHIP::Rebuild(Map *pMap) {
    if (!handle && orbt_localmap_create(device, &handle) != ORBX_OK) raise("LocalMapHIP::Rebuild");
    std::vector<KeyFrame *> vpKFs = pMap->GetAllKeyFrames();
    std::sort(vpKFs.begin(), vpKFs.end(), by_id);
    const std::vector<MapPoint *> vpMPs = pMap->GetAllMapPoints();
    T.Build(vpKFs, vpMPs);
    if (T.kfs.size() != vpKFs.size()) {   // an observer or a reference keyframe that the map no longer lists: it gets its slot and its features too
        vpKFs = T.kfs;
        T.Build(vpKFs, vpMPs);
    }
    const int K = T.table.K, P = T.table.P;
    index.clear();
    for (int p = 0; p < P; p++) index[T.pts[p]] = p;
    std::vector<int32_t> parent(K, -1), cov_off(1, 0), cov, child_off(1, 0), child;
    for (int s = 0; s < K; s++) {
        KeyFrame *k = T.kfs[s];
        std::map<KeyFrame *, int32_t>::const_iterator it;
        KeyFrame *pa = k->GetParent();
        if (pa && (it = T.slot.find(pa)) != T.slot.end()) parent[s] = it->second;
        const std::vector<KeyFrame *> vc = k->GetVectorCovisibleKeyFrames();
        for (size_t i = 0; i < vc.size(); i++)
            if ((it = T.slot.find(vc[i])) != T.slot.end()) cov.push_back(it->second);
        cov_off.push_back((int32_t)cov.size());
        const std::set<KeyFrame *> sc = k->GetChilds();
        const size_t c0 = child.size();
        for (std::set<KeyFrame *>::const_iterator sit = sc.begin(); sit != sc.end(); sit++)
            if ((it = T.slot.find(*sit)) != T.slot.end()) child.push_back(it->second);
        std::sort(child.begin() + c0, child.end());
        child_off.push_back((int32_t)child.size());
    }
    std::vector<orbt_pointview_t> views(P);
    std::vector<uint8_t> desc((size_t)32 * (P > 0 ? P : 1), 0);
    for (int p = 0; p < P; p++) {
        MapPoint *m = T.pts[p];
        for (int c = 0; c < 3; c++) views[p].normal[c] = m->mNormalVector.at<float>(c);
        // mfMaxDistance / mfMinDistance are protected in the reference's MapPoint.h: declare LocalMapHIP a friend there
        views[p].max_distance = m->mfMaxDistance; views[p].min_distance = m->mfMinDistance; views[p].observations = m->Observations();
        if (m->mDescriptor.rows > 0) std::memcpy(&desc[(size_t)32 * p], m->mDescriptor.ptr(0), 32);
    }
    orbt_map_t map;
    map.table = &T.table; map.features = &T.queries; map.parent = parent.data(); map.cov_off = cov_off.data(); map.cov = cov.data();
    map.child_off = child_off.data(); map.child = child.data(); map.views = views.data(); map.desc = desc.data();
    if (orbt_localmap_set_map(handle, &map) != ORBX_OK) raise("LocalMapHIP::Rebuild");
}

void Tracking::UpdateLocalMap() {
    LocalMapHIP &L = mLocalMap;
    if (!L.handle) L.Rebuild(mpMap);
    const int N = (int)mCurrentFrame.mvpMapPoints.size(), K = L.T.table.K, P = L.T.table.P;
    std::vector<int32_t> fp(N, -1), prev;
    std::vector<char> unknown(N, 0);
    for (int i = 0; i < N; i++) {
        MapPoint *pMP = mCurrentFrame.mvpMapPoints[i];
        if (!pMP) continue;
        std::map<MapPoint *, int32_t>::const_iterator it = L.index.find(pMP);
        if (it != L.index.end()) fp[i] = it->second;
        else unknown[i] = 1;
    }
    for (size_t j = 0; j < mvpLocalKeyFrames.size(); j++) {
        std::map<KeyFrame *, int32_t>::const_iterator it = L.T.slot.find(mvpLocalKeyFrames[j]);
        if (it != L.T.slot.end()) prev.push_back(it->second);
    }
    std::vector<int32_t> ofp(N);
    mHolder.assign(N, -1); mExtObs.assign(N, 0);
    // room for K keyframes and P points, grown when the snapshot grew and never cleared: a frame's cost does not grow with P
    if (mLkf.size() < (size_t)K + 1) mLkf.resize((size_t)K + 1);
    if (mLpts.size() < (size_t)P + 1) { mLpts.resize((size_t)P + 1); mLocalPts.resize((size_t)P + 1); mLocalDesc.resize((size_t)32 * (P + 1)); }
    std::vector<int32_t> &lkf = mLkf, &lpts = mLpts;
    orbt_local_t out;
    out.frame_points = ofp.data(); out.holder = mHolder.data(); out.ext_obs = mExtObs.data(); out.local_kf = lkf.data(); out.local_pts = lpts.data();
    out.pts = mLocalPts.data(); out.mp_desc = mLocalDesc.data();
    if (orbt_update_local_map(L.handle, fp.data(), N, prev.data(), (int)prev.size(), 80, 10, &out) != ORBX_OK) raise("Tracking::UpdateLocalMap");
    mLocalInfo = out.info;
    const long unsigned int id = mCurrentFrame.mnId;
    for (int i = 0; i < N; i++) {
        MapPoint *pMP = mCurrentFrame.mvpMapPoints[i];
        if (!pMP) continue;
        if (unknown[i]) {   // no observation, in no keyframe: a bad one is NULLed (:1391-1394), another stays outside the local map
            if (pMP->isBad()) mCurrentFrame.mvpMapPoints[i] = static_cast<MapPoint *>(NULL);
            else { mHolder[i] = -2; mExtObs[i] = pMP->Observations(); }
        } else if (ofp[i] < 0) mCurrentFrame.mvpMapPoints[i] = static_cast<MapPoint *>(NULL);
    }
    mvpLocalKeyFrames.resize(out.n_local_kf);
    for (int j = 0; j < out.n_local_kf; j++) {
        mvpLocalKeyFrames[j] = L.T.kfs[lkf[j]];
        if (!out.info.empty_vote) mvpLocalKeyFrames[j]->mnTrackReferenceForFrame = id;   // :1422, :1445, :1460, :1472
    }
    mvpLocalMapPoints.resize(out.n_local_pts);
    for (int j = 0; j < out.n_local_pts; j++) {
        mvpLocalMapPoints[j] = L.T.pts[lpts[j]];
        mvpLocalMapPoints[j]->mnTrackReferenceForFrame = id;   // :1369
    }
    if (out.info.ref_kf >= 0) {   // :1479-1483
        mpReferenceKF = L.T.kfs[out.info.ref_kf];
        mCurrentFrame.mpReferenceKF = mpReferenceKF;
    }
}

void Tracking::SearchLocalPoints() {
    Frame &F = mCurrentFrame;
    const int n = F.N, m = (int)mvpLocalMapPoints.size();
    mnMatchesLocal = 0; mnToMatch = 0;
    // Do not search map points already matched (:1291-1307)
    for (int i = 0; i < n; i++) {
        MapPoint *pMP = F.mvpMapPoints[i];
        if (!pMP) continue;
        if (pMP->isBad()) F.mvpMapPoints[i] = static_cast<MapPoint *>(NULL);
        else {
            pMP->IncreaseVisible();
            pMP->mnLastFrameSeen = F.mnId;
            pMP->mbTrackInView = false;
        }
    }
    if (m == 0) return;
    int th = 1;
    if (mSensor == System::RGBD) th = 3;
    if (F.mnId < mnLastRelocFrameId + 2) th = 5;   // :1330-1335
    std::vector<orbx_keypoint_t> kun(n > 0 ? n : 1);
    std::vector<uint8_t> desc((size_t)32 * (n > 0 ? n : 1));
    for (int i = 0; i < n; i++) {
        const cv::KeyPoint &k = F.mvKeysUn[i];
        kun[i].x = k.pt.x; kun[i].y = k.pt.y; kun[i].size = k.size; kun[i].angle = k.angle; kun[i].response = k.response; kun[i].octave = k.octave;
        kun[i].class_id = k.class_id;
        std::memcpy(&desc[(size_t)32 * i], F.mDescriptors.ptr(i), 32);
    }
    std::vector<int32_t> holder = mHolder;
    orbm_grid_geom_t g;
    g.min_x = Frame::mnMinX; g.min_y = Frame::mnMinY; g.max_x = Frame::mnMaxX; g.max_y = Frame::mnMaxY;
    g.inv_w = Frame::mfGridElementWidthInv; g.inv_h = Frame::mfGridElementHeightInv;
    orbm_camera_t cam;
    cam.fx = Frame::fx; cam.fy = Frame::fy; cam.cx = Frame::cx; cam.cy = Frame::cy; cam.mbf = F.mbf; cam.mb = F.mb;
    float Tcw[16], thr[16];
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) Tcw[r * 4 + c] = F.mTcw.at<float>(r, c);
    const int nlevels = (int)F.mvScaleFactors.size();
    if (nlevels > 16 || orbm_predict_scale_thresholds(F.mfLogScaleFactor, nlevels, thr) != ORBX_OK) raise("Tracking::SearchLocalPoints");
    std::vector<orbm_mappoint_t> proj(m);
    int nmatches = 0;
    if (orbm_search_local_points(kun.data(), desc.data(), F.mvuRight.data(), n, &g, F.mvScaleFactors.data(), nlevels, mLocalPts.data(), mLocalDesc.data(), m,
                                 Tcw, &cam, 0.5f, thr, holder.data(), mExtObs.data(), (float)th, 0.8f, ORBmatcher::device, &nmatches, proj.data()) != ORBX_OK)
        raise("Tracking::SearchLocalPoints");
    for (int i = 0; i < m; i++) {
        MapPoint *pMP = mvpLocalMapPoints[i];
        if (!mLocalPts[i].valid) continue;
        pMP->mbTrackInView = proj[i].in_view != 0;
        if (proj[i].in_view) {
            pMP->mTrackProjX = proj[i].proj_x; pMP->mTrackProjXR = proj[i].proj_xr; pMP->mTrackProjY = proj[i].proj_y;
            pMP->mnTrackScaleLevel = proj[i].level; pMP->mTrackViewCos = proj[i].view_cos;
            pMP->IncreaseVisible();   // :1320-1322
            mnToMatch++;
        }
    }
    for (int i = 0; i < n; i++)
        if (holder[i] != mHolder[i] && holder[i] >= 0) F.mvpMapPoints[i] = mvpLocalMapPoints[holder[i]];
    mnMatchesLocal = nmatches;
}

}  // namespace ORB_SLAM2
