// Optimizer.cc — see Optimizer.h.
#include "Optimizer.h"
#include <algorithm>
#include <cstdlib>
#include <list>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include "orbx.h"

namespace ORB_SLAM2 {

int Optimizer::device = std::getenv("ORBX_DEVICE") ? std::atoi(std::getenv("ORBX_DEVICE")) : 0;

int Optimizer::PoseOptimization(Frame *pFrame) {
    const int N = pFrame->N;
    std::vector<orbo_observation_t> obs((size_t)N);
    std::vector<uint8_t> outlier((size_t)N);
    for (int i = 0; i < N; i++) {
        orbo_observation_t &o = obs[i];
        MapPoint *pMP = pFrame->mvpMapPoints[i];
        outlier[i] = pFrame->mvbOutlier[i] ? 1 : 0;
        o.valid = pMP ? 1 : 0;
        const cv::KeyPoint &kpUn = pFrame->mvKeysUn[i];
        o.u = kpUn.pt.x; o.v = kpUn.pt.y; o.ur = pFrame->mvuRight[i];
        o.inv_sigma2 = pFrame->mvInvLevelSigma2[kpUn.octave];
        o.wx = o.wy = o.wz = 0.f;
        if (pMP) {
            cv::Mat Xw = pMP->GetWorldPos();
            o.wx = Xw.at<float>(0); o.wy = Xw.at<float>(1); o.wz = Xw.at<float>(2);
        }
    }
    const orbm_camera_t cam = {pFrame->fx, pFrame->fy, pFrame->cx, pFrame->cy, pFrame->mbf, pFrame->mb};
    float Tin[16], Tout[16];
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) Tin[r * 4 + c] = pFrame->mTcw.at<float>(r, c);
    int ngood = 0;
    orbo_pose_info_t info;
    const int rc = orbo_pose_optimization(obs.data(), N, &cam, Tin, Tout, outlier.data(), &ngood, &info, device);
    if (rc != ORBX_OK) throw std::runtime_error(std::string("Optimizer::PoseOptimization: ") + orbx_last_error());
    for (int i = 0; i < N; i++)
        if (obs[i].valid) pFrame->mvbOutlier[i] = outlier[i] != 0;
    if (info.correspondences < 3) return 0;   // :364-365: returns before the pose is written
    cv::Mat pose(4, 4, CV_32F);
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) pose.at<float>(r, c) = Tout[r * 4 + c];
    pFrame->SetPose(pose);
    return ngood;
}

int Optimizer::OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches1, g2o::Sim3 &g2oS12, const float th2,
                            const bool bFixScale) {
    orbz_sim3_problem_t prob;
    const cv::Mat &K1 = pKF1->mK;
    const cv::Mat &K2 = pKF2->mK;
    prob.K1[0] = K1.at<float>(0, 0); prob.K1[1] = K1.at<float>(1, 1); prob.K1[2] = K1.at<float>(0, 2); prob.K1[3] = K1.at<float>(1, 2);
    prob.K2[0] = K2.at<float>(0, 0); prob.K2[1] = K2.at<float>(1, 1); prob.K2[2] = K2.at<float>(0, 2); prob.K2[3] = K2.at<float>(1, 2);
    const cv::Mat T1 = pKF1->GetPose(), T2 = pKF2->GetPose();
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) { prob.Tcw1[r * 4 + c] = T1.at<float>(r, c); prob.Tcw2[r * 4 + c] = T2.at<float>(r, c); }
    const Eigen::Matrix3d R12 = g2oS12.rotation().toRotationMatrix();
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) prob.R[r * 3 + c] = (float)R12(r, c);
        prob.t[r] = (float)g2oS12.translation()[r];
    }
    prob.s = (float)g2oS12.scale();
    prob.th2 = th2;
    prob.fix_scale = bFixScale ? 1 : 0;

    const int N = (int)vpMatches1.size();
    const std::vector<MapPoint *> vpMapPoints1 = pKF1->GetMapPointMatches();
    std::vector<orbz_sim3_match_t> rows;
    std::vector<size_t> vnIndexEdge;
    rows.reserve(N); vnIndexEdge.reserve(N);
    for (int i = 0; i < N; i++) {   // :1104-1183
        if (!vpMatches1[i]) continue;
        MapPoint *pMP1 = vpMapPoints1[i];
        MapPoint *pMP2 = vpMatches1[i];
        const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
        if (!pMP1 || !pMP2) continue;
        if (pMP1->isBad() || pMP2->isBad() || i2 < 0) continue;
        orbz_sim3_match_t m;
        const cv::Mat P3D1w = pMP1->GetWorldPos(), P3D2w = pMP2->GetWorldPos();
        for (int k = 0; k < 3; k++) { m.w1[k] = P3D1w.at<float>(k); m.w2[k] = P3D2w.at<float>(k); }
        const cv::KeyPoint &kpUn1 = pKF1->mvKeysUn[i];
        const cv::KeyPoint &kpUn2 = pKF2->mvKeysUn[i2];
        m.u1 = kpUn1.pt.x; m.v1 = kpUn1.pt.y; m.u2 = kpUn2.pt.x; m.v2 = kpUn2.pt.y;
        m.inv_sigma2_1 = pKF1->mvInvLevelSigma2[kpUn1.octave];
        m.inv_sigma2_2 = pKF2->mvInvLevelSigma2[kpUn2.octave];
        rows.push_back(m);
        vnIndexEdge.push_back(i);
    }
    const int n = (int)rows.size();
    std::vector<uint8_t> dropped((size_t)n + 1, 0);
    float S12[16];
    int nIn = 0;
    orbz_sim3_info_t info;
    const int rc = orbz_optimize_sim3(rows.data(), n, &prob, S12, dropped.data(), &nIn, &info, device);
    if (rc != ORBX_OK) throw std::runtime_error(std::string("Optimizer::OptimizeSim3: ") + orbx_last_error());
    for (int k = 0; k < n; k++)
        if (dropped[k]) vpMatches1[vnIndexEdge[k]] = static_cast<MapPoint *>(NULL);
    if (info.rounds < 2) return 0;   // :1216-1217: returns before the vertex is read back
    g2oS12 = g2o::Sim3(Eigen::Quaterniond(info.q[3], info.q[0], info.q[1], info.q[2]), Eigen::Vector3d(info.t[0], info.t[1], info.t[2]), info.s);
    return nIn;
}

static int stop_flag_set(void *user) { return *(volatile bool *)user ? 1 : 0; }

static void fill_keyframe(orbb_keyframe_t &k, KeyFrame *pKF, bool fixed) {
    const cv::Mat T = pKF->GetPose();
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) k.Tcw[r * 4 + c] = T.at<float>(r, c);
    k.fx = pKF->fx; k.fy = pKF->fy; k.cx = pKF->cx; k.cy = pKF->cy; k.bf = pKF->mbf;
    k.fixed = fixed ? 1 : 0;
}
static orbb_observation_t make_observation(KeyFrame *pKFi, size_t idx, int kf, int pt) {
    const cv::KeyPoint &kpUn = pKFi->mvKeysUn[idx];
    orbb_observation_t o;
    o.kf = kf; o.pt = pt; o.u = kpUn.pt.x; o.v = kpUn.pt.y;
    o.ur = pKFi->mvuRight[idx] < 0 ? -1.f : pKFi->mvuRight[idx];
    o.inv_sigma2 = pKFi->mvInvLevelSigma2[kpUn.octave];
    return o;
}
static cv::Mat pose_mat(const float *T) {
    cv::Mat pose(4, 4, CV_32F);
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) pose.at<float>(r, c) = T[r * 4 + c];
    return pose;
}
static cv::Mat point_mat(const float *X) {
    cv::Mat pos(3, 1, CV_32F);
    for (int k = 0; k < 3; k++) pos.at<float>(k) = X[k];
    return pos;
}

void Optimizer::LocalBundleAdjustment(KeyFrame *pKF, bool *pbStopFlag, Map *pMap) {
    // Local KeyFrames: First Breath Search from Current Keyframe (:455-468)
    std::list<KeyFrame *> lLocalKeyFrames;
    lLocalKeyFrames.push_back(pKF);
    pKF->mnBALocalForKF = pKF->mnId;
    const std::vector<KeyFrame *> vNeighKFs = pKF->GetVectorCovisibleKeyFrames();
    for (int i = 0, iend = vNeighKFs.size(); i < iend; i++) {
        KeyFrame *pKFi = vNeighKFs[i];
        pKFi->mnBALocalForKF = pKF->mnId;
        if (!pKFi->isBad()) lLocalKeyFrames.push_back(pKFi);
    }
    // Local MapPoints seen in Local KeyFrames (:470-486)
    std::list<MapPoint *> lLocalMapPoints;
    for (std::list<KeyFrame *>::iterator lit = lLocalKeyFrames.begin(), lend = lLocalKeyFrames.end(); lit != lend; lit++) {
        std::vector<MapPoint *> vpMPs = (*lit)->GetMapPointMatches();
        for (std::vector<MapPoint *>::iterator vit = vpMPs.begin(), vend = vpMPs.end(); vit != vend; vit++) {
            MapPoint *pMP = *vit;
            if (pMP)
                if (!pMP->isBad())
                    if (pMP->mnBALocalForKF != pKF->mnId) {
                        lLocalMapPoints.push_back(pMP);
                        pMP->mnBALocalForKF = pKF->mnId;
                    }
        }
    }
    // Fixed Keyframes. Keyframes that see Local MapPoints but that are not Local Keyframes (:488-504)
    std::list<KeyFrame *> lFixedCameras;
    for (std::list<MapPoint *>::iterator lit = lLocalMapPoints.begin(), lend = lLocalMapPoints.end(); lit != lend; lit++) {
        std::map<KeyFrame *, size_t> observations = (*lit)->GetObservations();
        for (std::map<KeyFrame *, size_t>::iterator mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
            KeyFrame *pKFi = mit->first;
            if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
                pKFi->mnBAFixedForKF = pKF->mnId;
                if (!pKFi->isBad()) lFixedCameras.push_back(pKFi);
            }
        }
    }
    // the vertices (:522-546): the local keyframes, then the fixed ones
    std::vector<orbb_keyframe_t> kfs;
    std::map<KeyFrame *, int> index;
    for (std::list<KeyFrame *>::iterator lit = lLocalKeyFrames.begin(), lend = lLocalKeyFrames.end(); lit != lend; lit++) {
        orbb_keyframe_t k;
        fill_keyframe(k, *lit, (*lit)->mnId == 0);
        index[*lit] = (int)kfs.size();
        kfs.push_back(k);
    }
    for (std::list<KeyFrame *>::iterator lit = lFixedCameras.begin(), lend = lFixedCameras.end(); lit != lend; lit++) {
        orbb_keyframe_t k;
        fill_keyframe(k, *lit, true);
        index[*lit] = (int)kfs.size();
        kfs.push_back(k);
    }
    // the points and one edge per observation in a keyframe that is not bad (:572-653)
    std::vector<orbb_point_t> pts;
    std::vector<orbb_observation_t> obs;
    std::vector<KeyFrame *> vpEdgeKF;
    std::vector<MapPoint *> vpMapPointEdge;
    for (std::list<MapPoint *>::iterator lit = lLocalMapPoints.begin(), lend = lLocalMapPoints.end(); lit != lend; lit++) {
        MapPoint *pMP = *lit;
        const cv::Mat Xw = pMP->GetWorldPos();
        const orbb_point_t p = {Xw.at<float>(0), Xw.at<float>(1), Xw.at<float>(2)};
        const int id = (int)pts.size();
        pts.push_back(p);
        const std::map<KeyFrame *, size_t> observations = pMP->GetObservations();
        for (std::map<KeyFrame *, size_t>::const_iterator mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
            KeyFrame *pKFi = mit->first;
            if (pKFi->isBad() || !index.count(pKFi)) continue;
            obs.push_back(make_observation(pKFi, mit->second, index[pKFi], id));
            vpEdgeKF.push_back(pKFi);
            vpMapPointEdge.push_back(pMP);
        }
    }
    const int K = (int)kfs.size(), P = (int)pts.size(), E = (int)obs.size();
    std::vector<float> Tout((size_t)K * 16 + 1), Pout((size_t)P * 3 + 1);
    std::vector<uint8_t> erase((size_t)E + 1, 0);
    orbb_info_t info;
    const int rc = orbb_local_bundle_adjustment(kfs.data(), K, pts.data(), P, obs.data(), E, pbStopFlag ? stop_flag_set : NULL, pbStopFlag,
                                                Tout.data(), Pout.data(), erase.data(), &info, NULL, NULL, device);
    if (rc != ORBX_OK) throw std::runtime_error(std::string("Optimizer::LocalBundleAdjustment: ") + orbx_last_error());
    if (info.stopped_at == ORBB_STOP_BEFORE) return;   // :655-657
    // Get Map Mutex (:746-757)
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
    for (int e = 0; e < E; e++)
        if (erase[e]) {
            KeyFrame *pKFi = vpEdgeKF[e];
            MapPoint *pMPi = vpMapPointEdge[e];
            pKFi->EraseMapPointMatch(pMPi);
            pMPi->EraseObservation(pKFi);
        }
    // Recover optimized data (:759-779)
    for (std::list<KeyFrame *>::iterator lit = lLocalKeyFrames.begin(), lend = lLocalKeyFrames.end(); lit != lend; lit++) {
        KeyFrame *pKFl = *lit;
        pKFl->SetPose(pose_mat(Tout.data() + (size_t)index[pKFl] * 16));
#ifdef ORBX_HAVE_ORBSLAM2
        pMap->UpdateKeyFrame(pKFl);   // server keyframe
#endif
    }
    int id = 0;
    for (std::list<MapPoint *>::iterator lit = lLocalMapPoints.begin(), lend = lLocalMapPoints.end(); lit != lend; lit++, id++) {
        MapPoint *pMP = *lit;
        pMP->SetWorldPos(point_mat(Pout.data() + (size_t)id * 3));
        pMP->UpdateNormalAndDepth();
    }
}

void Optimizer::GlobalBundleAdjustemnt(Map *pMap, int nIterations, bool *pbStopFlag, const unsigned long nLoopKF, const bool bRobust) {
    std::vector<KeyFrame *> vpKFs = pMap->GetAllKeyFrames();
    std::vector<MapPoint *> vpMP = pMap->GetAllMapPoints();
    BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust);
}

void Optimizer::BundleAdjustment(const std::vector<KeyFrame *> &vpKFs, const std::vector<MapPoint *> &vpMP, int nIterations, bool *pbStopFlag,
                                 const unsigned long nLoopKF, const bool bRobust) {
    std::vector<orbb_keyframe_t> kfs;
    std::map<KeyFrame *, int> index;
    for (size_t i = 0; i < vpKFs.size(); i++) {   // :71-83
        KeyFrame *pKF = vpKFs[i];
        if (pKF->isBad()) continue;
        orbb_keyframe_t k;
        fill_keyframe(k, pKF, pKF->mnId == 0);
        index[pKF] = (int)kfs.size();
        kfs.push_back(k);
    }
    std::vector<orbb_point_t> pts;
    std::vector<orbb_observation_t> obs;
    std::vector<int> vnPoint(vpMP.size(), -1);   // -1: vbNotIncludedMP, or bad
    for (size_t i = 0; i < vpMP.size(); i++) {    // :89-184
        MapPoint *pMP = vpMP[i];
        if (pMP->isBad()) continue;
        const std::map<KeyFrame *, size_t> observations = pMP->GetObservations();
        const int id = (int)pts.size();
        int nEdges = 0;
        for (std::map<KeyFrame *, size_t>::const_iterator mit = observations.begin(); mit != observations.end(); mit++) {
            KeyFrame *pKF = mit->first;
            if (pKF->isBad() || !index.count(pKF)) continue;   // pKF->mnId > maxKFid: not among vpKFs
            nEdges++;
            obs.push_back(make_observation(pKF, mit->second, index[pKF], id));
        }
        if (nEdges == 0) continue;
        const cv::Mat Xw = pMP->GetWorldPos();
        const orbb_point_t p = {Xw.at<float>(0), Xw.at<float>(1), Xw.at<float>(2)};
        pts.push_back(p);
        vnPoint[i] = id;
    }
    const int K = (int)kfs.size(), P = (int)pts.size(), E = (int)obs.size();
    std::vector<float> Tout((size_t)K * 16 + 1), Pout((size_t)P * 3 + 1);
    if (nLoopKF != 0) {
        // The loop closer's adjustment of the whole map (src/LoopClosing.cc:659): the blocked reduced-system path, and the write-back of
        // :204-209 and :229-234 - the results go beside the map (mTcwGBA, mPosGBA) with the mnBAGlobalForKF mark, the map itself is
        // left as it is for LoopClosing::RunGlobalBundleAdjustment to correct under its own lock
        const int rcg = orbb_global_bundle_adjustment(kfs.data(), K, pts.data(), P, obs.data(), E, nIterations, bRobust ? 1 : 0,
                                                      pbStopFlag ? stop_flag_set : NULL, pbStopFlag, Tout.data(), Pout.data(), NULL, NULL, NULL, NULL, device);
        if (rcg != ORBX_OK) throw std::runtime_error(std::string("Optimizer::BundleAdjustment: ") + orbx_last_error());
        for (size_t i = 0; i < vpKFs.size(); i++) {
            KeyFrame *pKF = vpKFs[i];
            if (pKF->isBad()) continue;
            pKF->mTcwGBA = pose_mat(Tout.data() + (size_t)index[pKF] * 16);
            pKF->mnBAGlobalForKF = nLoopKF;
        }
        for (size_t i = 0; i < vpMP.size(); i++) {
            if (vnPoint[i] < 0) continue;
            vpMP[i]->mPosGBA = point_mat(Pout.data() + (size_t)vnPoint[i] * 3);
            vpMP[i]->mnBAGlobalForKF = nLoopKF;
        }
        return;
    }
    const int rc = orbb_bundle_adjustment(kfs.data(), K, pts.data(), P, obs.data(), E, nIterations, bRobust ? 1 : 0, pbStopFlag ? stop_flag_set : NULL,
                                          pbStopFlag, Tout.data(), Pout.data(), NULL, NULL, NULL, device);
    if (rc != ORBX_OK) throw std::runtime_error(std::string("Optimizer::BundleAdjustment: ") + orbx_last_error());
    for (size_t i = 0; i < vpKFs.size(); i++) {   // :193-210
        KeyFrame *pKF = vpKFs[i];
        if (pKF->isBad()) continue;
        pKF->SetPose(pose_mat(Tout.data() + (size_t)index[pKF] * 16));
    }
    for (size_t i = 0; i < vpMP.size(); i++) {    // :213-235
        if (vnPoint[i] < 0) continue;
        MapPoint *pMP = vpMP[i];
        pMP->SetWorldPos(point_mat(Pout.data() + (size_t)vnPoint[i] * 3));
        pMP->UpdateNormalAndDepth();
    }
}

// ---- OptimizeEssentialGraph (src/Optimizer.cc:783-1049) ----------------------------------------------------------------------------
static orbg_sim3_t flat_sim3(const g2o::Sim3 &S) {
    orbg_sim3_t o;
    o.q[0] = S.rotation().x(); o.q[1] = S.rotation().y(); o.q[2] = S.rotation().z(); o.q[3] = S.rotation().w();
    for (int k = 0; k < 3; k++) o.t[k] = S.translation()[k];
    o.s = S.scale();
    return o;
}
static bool by_mnid(KeyFrame *a, KeyFrame *b) { return a->mnId < b->mnId; }
static std::vector<KeyFrame *> sorted_by_mnid(const std::set<KeyFrame *> &s) {   // the reference walks such a set in pointer order
    std::vector<KeyFrame *> v(s.begin(), s.end());
    std::sort(v.begin(), v.end(), by_mnid);
    return v;
}

void Optimizer::OptimizeEssentialGraph(Map *pMap, KeyFrame *pLoopKF, KeyFrame *pCurKF, const LoopClosing::KeyFrameAndPose &NonCorrectedSim3,
                                       const LoopClosing::KeyFrameAndPose &CorrectedSim3,
                                       const std::map<KeyFrame *, std::set<KeyFrame *> > &LoopConnections, const bool &bFixScale) {
    const std::vector<KeyFrame *> vpKFs = pMap->GetAllKeyFrames();
    const std::vector<MapPoint *> vpMPs = pMap->GetAllMapPoints();
    const int minFeat = 100;
    // Set KeyFrame vertices (:811-846): mnId -> dense vertex index, a bad keyframe has none
    std::map<KeyFrame *, int> vertexOf;
    std::map<unsigned long, int> vertexOfId;
    std::vector<orbg_vertex_t> vertices;
    for (size_t i = 0; i < vpKFs.size(); i++) {
        KeyFrame *pKF = vpKFs[i];
        if (pKF->isBad()) continue;
        orbg_vertex_t v;
        LoopClosing::KeyFrameAndPose::const_iterator it = CorrectedSim3.find(pKF);
        if (it != CorrectedSim3.end()) v.Scw = flat_sim3(it->second);
        else v.Scw = flat_sim3(g2o::Sim3(Converter::toMatrix3d(pKF->GetRotation()), Converter::toVector3d(pKF->GetTranslation()), 1.0));
        LoopClosing::KeyFrameAndPose::const_iterator itn = NonCorrectedSim3.find(pKF);
        v.has_nc = itn != NonCorrectedSim3.end() ? 1 : 0;
        v.Snc = v.has_nc ? flat_sim3(itn->second) : v.Scw;
        v.fixed = pKF == pLoopKF ? 1 : 0;
        vertexOf[pKF] = (int)vertices.size();
        vertexOfId[pKF->mnId] = (int)vertices.size();
        vertices.push_back(v);
    }
    std::vector<orbg_edge_t> edges;
    std::set<std::pair<long unsigned int, long unsigned int> > sInsertedEdges;
    // Set Loop edges (:854-882), the map's keys and every set in ascending mnId
    std::vector<KeyFrame *> keys;
    for (std::map<KeyFrame *, std::set<KeyFrame *> >::const_iterator mit = LoopConnections.begin(); mit != LoopConnections.end(); mit++) keys.push_back(mit->first);
    std::sort(keys.begin(), keys.end(), by_mnid);
    for (size_t k = 0; k < keys.size(); k++) {
        KeyFrame *pKF = keys[k];
        const long unsigned int nIDi = pKF->mnId;
        const std::vector<KeyFrame *> conn = sorted_by_mnid(LoopConnections.find(pKF)->second);
        for (size_t c = 0; c < conn.size(); c++) {
            const long unsigned int nIDj = conn[c]->mnId;
            if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(conn[c]) < minFeat) continue;
            if (!vertexOf.count(pKF) || !vertexOf.count(conn[c])) continue;   // a bad keyframe: the reference would hand g2o a null vertex
            const orbg_edge_t e = {vertexOf[pKF], vertexOf[conn[c]], 0};
            edges.push_back(e);
            sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
        }
    }
    // Set normal edges (:885-985)
    for (size_t i = 0; i < vpKFs.size(); i++) {
        KeyFrame *pKF = vpKFs[i];
        if (!vertexOf.count(pKF)) continue;
        const int vi = vertexOf[pKF];
        KeyFrame *pParentKF = pKF->GetParent();
        if (pParentKF && vertexOf.count(pParentKF)) {   // spanning tree edge
            const orbg_edge_t e = {vi, vertexOf[pParentKF], 1};
            edges.push_back(e);
        }
        const std::set<KeyFrame *> sLoopEdges = pKF->GetLoopEdges();
        const std::vector<KeyFrame *> vLoop = sorted_by_mnid(sLoopEdges);
        for (size_t l = 0; l < vLoop.size(); l++)
            if (vLoop[l]->mnId < pKF->mnId && vertexOf.count(vLoop[l])) {
                const orbg_edge_t e = {vi, vertexOf[vLoop[l]], 1};
                edges.push_back(e);
            }
        const std::vector<KeyFrame *> vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);
        for (std::vector<KeyFrame *>::const_iterator vit = vpConnectedKFs.begin(); vit != vpConnectedKFs.end(); vit++) {
            KeyFrame *pKFn = *vit;
            if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn)) {
                if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
                    if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
                    if (!vertexOf.count(pKFn)) continue;
                    const orbg_edge_t e = {vi, vertexOf[pKFn], 1};
                    edges.push_back(e);
                }
            }
        }
    }
    // the points of :1018-1048; one whose reference keyframe has no vertex is left as it is (the reference reads a default Sim3 there)
    std::vector<orbg_point_t> points;
    std::vector<MapPoint *> moved;
    for (size_t i = 0; i < vpMPs.size(); i++) {
        MapPoint *pMP = vpMPs[i];
        if (pMP->isBad()) continue;
        unsigned long nIDr;
        if (pMP->mnCorrectedByKF == pCurKF->mnId) nIDr = pMP->mnCorrectedReference;
        else {
            KeyFrame *pRefKF = pMP->GetReferenceKeyFrame();
            if (!pRefKF) continue;
            nIDr = pRefKF->mnId;
        }
        if (!vertexOfId.count(nIDr)) continue;
        const cv::Mat P3Dw = pMP->GetWorldPos();
        const orbg_point_t p = {P3Dw.at<float>(0), P3Dw.at<float>(1), P3Dw.at<float>(2), vertexOfId[nIDr]};
        points.push_back(p);
        moved.push_back(pMP);
    }
    const int N = (int)vertices.size(), E = (int)edges.size(), P = (int)points.size();
    std::vector<float> Tout((size_t)N * 16 + 1), Pout((size_t)P * 3 + 1);
    const int rc = orbg_optimize_essential_graph(vertices.data(), N, edges.data(), E, points.data(), P, bFixScale ? 1 : 0, 20, Tout.data(), Pout.data(),
                                                 NULL, NULL, device);
    if (rc != ORBX_OK) throw std::runtime_error(std::string("Optimizer::OptimizeEssentialGraph: ") + orbx_last_error());
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
    // SE3 pose recovering (:994-1015), a bad keyframe skipped (the reference dereferences its missing vertex); UpdateKeyFrame of the
    // multi-agent server is the caller's
    for (size_t i = 0; i < vpKFs.size(); i++)
        if (vertexOf.count(vpKFs[i])) vpKFs[i]->SetPose(pose_mat(Tout.data() + (size_t)vertexOf[vpKFs[i]] * 16));
    for (size_t i = 0; i < moved.size(); i++) {
        moved[i]->SetWorldPos(point_mat(Pout.data() + i * 3));
        moved[i]->UpdateNormalAndDepth();
    }
}

}  // namespace ORB_SLAM2
