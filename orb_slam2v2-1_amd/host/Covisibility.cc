// Covisibility.cc — the covisibility calls of include/orbx.h over the shim's objects (see Covisibility.h).
#include "Covisibility.h"
#include <algorithm>
#include <cstdlib>
#include <stdexcept>
#include <string>

namespace ORB_SLAM2 {

int Covisibility::device = std::getenv("ORBX_DEVICE") ? std::atoi(std::getenv("ORBX_DEVICE")) : 0;

namespace {
bool by_id(KeyFrame *a, KeyFrame *b) { return a->mnId != b->mnId ? a->mnId < b->mnId : a < b; }
}

void CovisTables::Build(const std::vector<KeyFrame *> &vpQueries, const std::vector<MapPoint *> &vpPoints) {
    kfs.clear(); slot.clear(); pts.clear(); kf.clear(); pt.clear(); obs_off.clear(); query_kf.clear(); feat_off.clear(); obs.clear(); feat.clear(); sf.clear();
    std::map<MapPoint *, int32_t> index;
    for (size_t i = 0; i < vpPoints.size(); i++)
        if (vpPoints[i] && !index.count(vpPoints[i])) { index[vpPoints[i]] = (int32_t)pts.size(); pts.push_back(vpPoints[i]); }
    for (size_t q = 0; q < vpQueries.size(); q++) {
        const std::vector<MapPoint *> &v = vpQueries[q]->mvpMapPoints;
        for (size_t i = 0; i < v.size(); i++)
            if (v[i] && !index.count(v[i])) { index[v[i]] = (int32_t)pts.size(); pts.push_back(v[i]); }
    }
    std::set<KeyFrame *> all(vpQueries.begin(), vpQueries.end());
    for (size_t p = 0; p < pts.size(); p++) {
        for (std::map<KeyFrame *, size_t>::iterator mit = pts[p]->mObservations.begin(), mend = pts[p]->mObservations.end(); mit != mend; mit++) all.insert(mit->first);
        if (pts[p]->mpRefKF) all.insert(pts[p]->mpRefKF);
    }
    kfs.assign(all.begin(), all.end());
    std::sort(kfs.begin(), kfs.end(), by_id);
    kf.resize(kfs.size());
    for (size_t s = 0; s < kfs.size(); s++) {
        KeyFrame *k = kfs[s];
        slot[k] = (int32_t)s;
        orbc_keyframe_t &r = kf[s];
        r.id = (int32_t)k->mnId; r.bad = k->mbBad; r.not_erase = k->mbNotErase; r.pad[0] = r.pad[1] = 0; r.th_depth = k->mThDepth;
        for (int c = 0; c < 3; c++) r.Ow[c] = k->Ow.at<float>(c);
        if (sf.empty() && !k->mvScaleFactors.empty()) sf = k->mvScaleFactors;   // every keyframe copies the one extractor's table
    }
    if (sf.empty()) sf.assign(1, 1.f);
    pt.resize(pts.size());
    obs_off.assign(1, 0);
    for (size_t p = 0; p < pts.size(); p++) {
        MapPoint *m = pts[p];
        orbc_point_t &r = pt[p];
        for (int c = 0; c < 3; c++) r.pos[c] = m->mWorldPos.at<float>(c);
        r.ref_kf = m->mpRefKF ? slot[m->mpRefKF] : -1; r.bad = m->mbBad; r.pad[0] = r.pad[1] = r.pad[2] = 0;
        std::vector<orbc_observation_t> mine;
        for (std::map<KeyFrame *, size_t>::iterator mit = m->mObservations.begin(), mend = m->mObservations.end(); mit != mend; mit++) {
            KeyFrame *k = mit->first;
            orbc_observation_t o;
            o.kf = slot[k]; o.idx = (int32_t)mit->second; o.pad[0] = o.pad[1] = 0;
            o.octave = mit->second < k->mvKeysUn.size() ? (uint8_t)k->mvKeysUn[mit->second].octave : 0;
            o.stereo = mit->second < k->mvuRight.size() && k->mvuRight[mit->second] >= 0;
            mine.push_back(o);
        }
        std::sort(mine.begin(), mine.end(), [](const orbc_observation_t &a, const orbc_observation_t &b) { return a.kf < b.kf; });
        obs.insert(obs.end(), mine.begin(), mine.end());
        obs_off.push_back((int32_t)obs.size());
    }
    feat_off.assign(1, 0);
    for (size_t q = 0; q < vpQueries.size(); q++) {
        KeyFrame *k = vpQueries[q];
        query_kf.push_back(slot[k]);
        for (size_t i = 0; i < k->mvpMapPoints.size(); i++) {
            orbc_feature_t f;
            f.point = k->mvpMapPoints[i] ? index[k->mvpMapPoints[i]] : -1;
            f.octave = i < k->mvKeysUn.size() ? k->mvKeysUn[i].octave : 0;
            f.depth = i < k->mvDepth.size() ? k->mvDepth[i] : -1.f;
            feat.push_back(f);
        }
        feat_off.push_back((int32_t)feat.size());
    }
    table.kf = kf.data(); table.K = (int32_t)kf.size(); table.pts = pt.data(); table.P = (int32_t)pt.size(); table.obs_off = obs_off.data();
    table.obs = obs.data(); table.scale_factors = sf.data(); table.nlevels = (int32_t)sf.size();
    queries.query_kf = query_kf.data(); queries.Q = (int32_t)query_kf.size(); queries.feat_off = feat_off.data(); queries.feat = feat.data();
}

namespace {
// KeyFrame::UpdateBestCovisibles (src/KeyFrame.cc:139-161) with mnId for the pointer
void update_best_covisibles(KeyFrame *k) {
    std::vector<std::pair<int, KeyFrame *> > v;
    for (std::map<KeyFrame *, int>::iterator mit = k->mConnectedKeyFrameWeights.begin(), mend = k->mConnectedKeyFrameWeights.end(); mit != mend; mit++)
        v.push_back(std::make_pair(mit->second, mit->first));
    std::sort(v.begin(), v.end(), [](const std::pair<int, KeyFrame *> &a, const std::pair<int, KeyFrame *> &b) {
        return a.first != b.first ? a.first < b.first : by_id(a.second, b.second);
    });
    k->mvpOrderedConnectedKeyFrames.clear(); k->mvOrderedWeights.clear();
    for (size_t i = v.size(); i-- > 0;) { k->mvpOrderedConnectedKeyFrames.push_back(v[i].second); k->mvOrderedWeights.push_back(v[i].first); }
}
// KeyFrame::AddConnection (src/KeyFrame.cc:123-137)
void add_connection(KeyFrame *k, KeyFrame *pKF, int weight) {
    std::map<KeyFrame *, int>::iterator it = k->mConnectedKeyFrameWeights.find(pKF);
    if (it == k->mConnectedKeyFrameWeights.end()) k->mConnectedKeyFrameWeights[pKF] = weight;
    else if (it->second != weight) it->second = weight;
    else return;
    update_best_covisibles(k);
}
}  // namespace

void UpdateConnectionsHIP(const std::vector<KeyFrame *> &vpKFs) {
    if (vpKFs.empty()) return;
    CovisTables T;
    T.Build(vpKFs, std::vector<MapPoint *>());
    UpdateConnectionsHIP(T, vpKFs);
}

void UpdateConnectionsHIP(CovisTables &T, const std::vector<KeyFrame *> &vpKFs) {
    if (vpKFs.empty()) return;
    const int Q = (int)vpKFs.size(), K = T.table.K;
    std::vector<int32_t> ids((size_t)Q * K), ws((size_t)Q * K), n(Q), counters((size_t)Q * K);
    if (orbc_update_connections(&T.table, &T.queries, 15, K, ids.data(), ws.data(), n.data(), counters.data(), Covisibility::device) != ORBX_OK)
        throw std::runtime_error(std::string("UpdateConnectionsHIP: ") + orbx_last_error());
    for (int q = 0; q < Q; q++) {
        if (n[q] == 0) continue;   // :324-325
        KeyFrame *me = vpKFs[q];
        for (int i = 0; i < n[q]; i++) add_connection(T.kfs[ids[(size_t)q * K + i]], me, ws[(size_t)q * K + i]);   // :345, :352
        me->mConnectedKeyFrameWeights.clear();
        for (int k = 0; k < K; k++)
            if (counters[(size_t)q * K + k]) me->mConnectedKeyFrameWeights[T.kfs[k]] = counters[(size_t)q * K + k];
        me->mvpOrderedConnectedKeyFrames.clear(); me->mvOrderedWeights.clear();
        for (int i = 0; i < n[q]; i++) { me->mvpOrderedConnectedKeyFrames.push_back(T.kfs[ids[(size_t)q * K + i]]); me->mvOrderedWeights.push_back(ws[(size_t)q * K + i]); }
    }
}

void UpdateNormalAndDepthHIP(const std::vector<MapPoint *> &vpMPs) {
    if (vpMPs.empty()) return;
    CovisTables T;
    T.Build(std::vector<KeyFrame *>(), vpMPs);
    std::vector<orbc_normal_t> out(T.pts.size());
    if (orbc_update_normal_and_depth(&T.table, out.data(), Covisibility::device) != ORBX_OK)
        throw std::runtime_error(std::string("UpdateNormalAndDepthHIP: ") + orbx_last_error());
    for (size_t p = 0; p < T.pts.size(); p++) {
        if (out[p].status != ORBC_NORMAL_OK) continue;
        MapPoint *m = T.pts[p];
        m->mfMaxDistance = out[p].max_distance; m->mfMinDistance = out[p].min_distance;
        for (int c = 0; c < 3; c++) m->mNormalVector.at<float>(c) = out[p].normal[c];
    }
}

}  // namespace ORB_SLAM2
