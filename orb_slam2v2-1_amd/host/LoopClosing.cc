// LoopClosing.cc — the loop map correction calls of include/orbx.h over the shim's objects (see LoopClosing.h).
#include "LoopClosing.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <set>
#include <stdexcept>
#include <string>
#include "Covisibility.h"
#include "orbx.h"

namespace ORB_SLAM2 {

int LoopClosing::device = std::getenv("ORBX_DEVICE") ? std::atoi(std::getenv("ORBX_DEVICE")) : 0;

namespace {
bool by_id(KeyFrame *a, KeyFrame *b) { return a->mnId != b->mnId ? a->mnId < b->mnId : a < b; }
void pose16(const cv::Mat &T, float *out) {
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) out[r * 4 + c] = T.at<float>(r, c);
}
cv::Mat mat44(const float *p) {
    cv::Mat T(4, 4, CV_32F);
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) T.at<float>(r, c) = p[r * 4 + c];
    return T;
}
cv::Mat mat31(const float *p) {
    cv::Mat v(3, 1, CV_32F);
    for (int c = 0; c < 3; c++) v.at<float>(c) = p[c];
    return v;
}
g2o::Sim3 sim3_of(const orbg_sim3_t &s) {
    return g2o::Sim3(Eigen::Quaterniond(s.q[3], s.q[0], s.q[1], s.q[2]), Eigen::Vector3d(s.t[0], s.t[1], s.t[2]), s.s);
}
}  // namespace

void LoopClosing::CorrectLoopPoses(KeyFrameAndPose &CorrectedSim3, KeyFrameAndPose &NonCorrectedSim3) {
    mvpCurrentConnectedKFs = mpCurrentKF->GetVectorCovisibleKeyFrames();   // :445-446
    mvpCurrentConnectedKFs.push_back(mpCurrentKF);
    std::vector<KeyFrame *> queries(mvpCurrentConnectedKFs);
    std::sort(queries.begin(), queries.end(), by_id);   // the table's slots ascend in mnId: so do the queries' then
    queries.erase(std::unique(queries.begin(), queries.end()), queries.end());
    CovisTables T;
    T.Build(queries, std::vector<MapPoint *>());
    const int Q = (int)queries.size(), P = T.table.P;
    std::vector<float> Tiw((size_t)Q * 16), Tnew((size_t)Q * 16), Ow((size_t)Q * 3), pos((size_t)P * 3 + 1);
    for (int q = 0; q < Q; q++) pose16(queries[q]->GetPose(), &Tiw[(size_t)q * 16]);
    orbg_sim3_t Scw;
    Scw.q[0] = mg2oScw.rotation().x(); Scw.q[1] = mg2oScw.rotation().y(); Scw.q[2] = mg2oScw.rotation().z(); Scw.q[3] = mg2oScw.rotation().w();
    for (int c = 0; c < 3; c++) Scw.t[c] = mg2oScw.translation()[c];
    Scw.s = mg2oScw.scale();
    std::vector<orbg_sim3_t> corrected(Q), non_corrected(Q);
    std::vector<int32_t> ref((size_t)P + 1);
    std::vector<orbc_normal_t> normals((size_t)P + 1);
    const orbr_loop_out_t out = {corrected.data(), non_corrected.data(), Tnew.data(), Ow.data(), pos.data(), ref.data(), normals.data()};
    if (orbr_correct_loop(&T.table, &T.queries, T.slot[mpCurrentKF], Tiw.data(), &Scw, &out, device) != ORBX_OK)
        throw std::runtime_error(std::string("LoopClosing::CorrectLoopPoses: ") + orbx_last_error());
    for (int q = 0; q < Q; q++) {
        CorrectedSim3[queries[q]] = sim3_of(corrected[q]);          // :449, :471
        NonCorrectedSim3[queries[q]] = sim3_of(non_corrected[q]);   // :478
    }
    for (int p = 0; p < P; p++) {
        if (ref[p] < 0) continue;
        MapPoint *m = T.pts[p];
        m->SetWorldPos(mat31(&pos[(size_t)p * 3]));                 // :507-509
        m->mnCorrectedByKF = mpCurrentKF->mnId;
        m->mnCorrectedReference = T.kfs[ref[p]]->mnId;
        if (normals[p].status != ORBC_NORMAL_OK) continue;          // :510
        m->mfMaxDistance = normals[p].max_distance; m->mfMinDistance = normals[p].min_distance;
        for (int c = 0; c < 3; c++) m->mNormalVector.at<float>(c) = normals[p].normal[c];
    }
    for (int q = 0; q < Q; q++) queries[q]->SetPose(mat44(&Tnew[(size_t)q * 16]));   // :522
    UpdateConnectionsHIP(T, queries);                               // :524
}

void LoopClosing::UpdateMapAfterGlobalBA(unsigned long nLoopKF) {
    // every keyframe the walk or a point can name: the map's, the origins, all their descendants and the reference keyframes
    std::set<KeyFrame *> all;
    std::vector<KeyFrame *> work = mpMap->GetAllKeyFrames();
    work.insert(work.end(), mpMap->mvpKeyFrameOrigins.begin(), mpMap->mvpKeyFrameOrigins.end());
    const std::vector<MapPoint *> vpMPs = mpMap->GetAllMapPoints();
    for (size_t i = 0; i < vpMPs.size(); i++)
        if (vpMPs[i]->GetReferenceKeyFrame()) work.push_back(vpMPs[i]->GetReferenceKeyFrame());
    while (!work.empty()) {
        KeyFrame *k = work.back();
        work.pop_back();
        if (!all.insert(k).second) continue;
        const std::set<KeyFrame *> ch = k->GetChilds();
        work.insert(work.end(), ch.begin(), ch.end());
    }
    std::vector<KeyFrame *> kfs(all.begin(), all.end());
    std::sort(kfs.begin(), kfs.end(), by_id);
    std::map<KeyFrame *, int32_t> slot;
    for (size_t s = 0; s < kfs.size(); s++) slot[kfs[s]] = (int32_t)s;
    const int K = (int)kfs.size(), P = (int)vpMPs.size();
    std::vector<float> Tcw((size_t)K * 16 + 1), gba((size_t)K * 16 + 1, 0.f), Tnew((size_t)K * 16 + 1), gbaOut((size_t)K * 16 + 1);
    std::vector<uint8_t> in_gba((size_t)K + 1), marked((size_t)K + 1), reached((size_t)K + 1);
    std::vector<int32_t> child_off(1, 0), child, origins;
    for (int s = 0; s < K; s++) {
        KeyFrame *k = kfs[s];
        pose16(k->GetPose(), &Tcw[(size_t)s * 16]);
        in_gba[s] = k->mnBAGlobalForKF == nLoopKF;
        if (in_gba[s] && !k->mTcwGBA.empty()) pose16(k->mTcwGBA, &gba[(size_t)s * 16]);
        const std::set<KeyFrame *> ch = k->GetChilds();
        std::vector<int32_t> mine;
        for (std::set<KeyFrame *>::const_iterator sit = ch.begin(); sit != ch.end(); sit++) mine.push_back(slot[*sit]);
        std::sort(mine.begin(), mine.end());
        child.insert(child.end(), mine.begin(), mine.end());
        child_off.push_back((int32_t)child.size());
    }
    for (size_t i = 0; i < mpMap->mvpKeyFrameOrigins.size(); i++) origins.push_back(slot[mpMap->mvpKeyFrameOrigins[i]]);
    std::vector<float> pos((size_t)P * 3 + 1), posGBA((size_t)P * 3 + 1, 0.f), posOut((size_t)P * 3 + 1);
    std::vector<uint8_t> pt_in((size_t)P + 1), bad((size_t)P + 1);
    std::vector<int32_t> refkf((size_t)P + 1), status((size_t)P + 1);
    for (int p = 0; p < P; p++) {
        MapPoint *m = vpMPs[p];
        for (int c = 0; c < 3; c++) pos[(size_t)p * 3 + c] = m->mWorldPos.at<float>(c);
        pt_in[p] = m->mnBAGlobalForKF == nLoopKF;
        if (pt_in[p] && !m->mPosGBA.empty())
            for (int c = 0; c < 3; c++) posGBA[(size_t)p * 3 + c] = m->mPosGBA.at<float>(c);
        bad[p] = m->isBad();
        refkf[p] = m->GetReferenceKeyFrame() ? slot[m->GetReferenceKeyFrame()] : -1;
    }
    child.push_back(0); origins.push_back(0);   // never empty: data() is a pointer
    orbr_spread_in_t in;
    in.K = K; in.Tcw16 = Tcw.data(); in.TcwGBA16 = gba.data(); in.kf_in_gba = in_gba.data(); in.child_off = child_off.data(); in.child = child.data();
    in.origins = origins.data(); in.n_origins = (int32_t)origins.size() - 1; in.P = P; in.pos3 = pos.data(); in.posGBA3 = posGBA.data();
    in.pt_in_gba = pt_in.data(); in.ref_kf = refkf.data(); in.bad = bad.data();
    orbr_spread_out_t out;
    out.Tcw_new16 = Tnew.data(); out.TcwGBA_out16 = gbaOut.data(); out.kf_marked = marked.data(); out.kf_reached = reached.data();
    out.pos_out3 = posOut.data(); out.status = status.data(); out.levels = 0;
    if (orbr_spread_global_ba(&in, &out, device) != ORBX_OK)
        throw std::runtime_error(std::string("LoopClosing::UpdateMapAfterGlobalBA: ") + orbx_last_error());
    for (int s = 0; s < K; s++) {
        if (!reached[s]) continue;
        KeyFrame *k = kfs[s];
        if (!in_gba[s]) { k->mTcwGBA = mat44(&gbaOut[(size_t)s * 16]); k->mnBAGlobalForKF = nLoopKF; }   // :699-700
        k->mTcwBefGBA = k->GetPose();                    // :706
        k->SetPose(mat44(&Tnew[(size_t)s * 16]));        // :707
    }
    for (int p = 0; p < P; p++)
        if (status[p] == ORBR_SPREAD_GBA || status[p] == ORBR_SPREAD_MOVED) vpMPs[p]->SetWorldPos(mat31(&posOut[(size_t)p * 3]));   // :724, :744
}

}  // namespace ORB_SLAM2
