// LocalMapping.cc — ORB_SLAM2::LocalMapping::CreateNewMapPoints and KeyFrameCulling over include/orbx.h (see LocalMapping.h).
#include "LocalMapping.h"
#include "Covisibility.h"
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include "orbx.h"

namespace ORB_SLAM2 {

int LocalMapping::device = std::getenv("ORBX_DEVICE") ? std::atoi(std::getenv("ORBX_DEVICE")) : 0;

namespace {
// what orbl_create_new_map_points reads of one keyframe, gathered into arrays that outlive the call
struct Side {
    orbl_view_t view;
    std::vector<orbx_keypoint_t> kp;
    std::vector<orbl_stereo_t> st;
    std::vector<uint8_t> desc, flags;
    orbl_keyframe_t kf;
    void gather(KeyFrame *pKF) {
        std::memset(&view, 0, sizeof(view));
        const cv::Mat T = pKF->GetPose(), Ow = pKF->GetCameraCenter();
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) view.Tcw[r * 4 + c] = T.at<float>(r, c);
        for (int k = 0; k < 3; k++) view.Ow[k] = Ow.at<float>(k);
        view.fx = pKF->fx; view.fy = pKF->fy; view.cx = pKF->cx; view.cy = pKF->cy; view.invfx = pKF->invfx; view.invfy = pKF->invfy;
        view.mb = pKF->mb; view.mbf = pKF->mbf; view.scale_factor = pKF->mfScaleFactor; view.nlevels = (int32_t)pKF->mvScaleFactors.size();
        const int n = pKF->N;
        kp.resize(n); st.resize(n); flags.resize(n); desc.resize((size_t)32 * (n > 0 ? n : 1));
        for (int i = 0; i < n; i++) {
            const cv::KeyPoint &k = pKF->mvKeysUn[i];
            kp[i].x = k.pt.x; kp[i].y = k.pt.y; kp[i].size = k.size; kp[i].angle = k.angle; kp[i].response = k.response; kp[i].octave = k.octave;
            kp[i].class_id = k.class_id;
            const bool stereo = pKF->mvuRight[i] >= 0;
            st[i].ur = pKF->mvuRight[i]; st[i].depth = pKF->mvDepth[i]; st[i].raw_u = pKF->mvKeys[i].pt.x; st[i].raw_v = pKF->mvKeys[i].pt.y;
            flags[i] = (uint8_t)((!pKF->GetMapPoint(i) ? 1 : 0) | (stereo ? 2 : 0));   // src/ORBmatcher.cc:700-710, :721-731 with bOnlyStereo false
            std::memcpy(&desc[(size_t)32 * i], pKF->mDescriptors.ptr(i), 32);
        }
        kf.view = &view; kf.kp = kp.data(); kf.st = st.data(); kf.n = n;
        kf.scale_factors = pKF->mvScaleFactors.data(); kf.level_sigma2 = pKF->mvLevelSigma2.data();
    }
};
struct Lists { std::vector<int32_t> sq, iq, sc, ic; };
// the merge of the two FeatureVectors, as ORBmatcher::SearchForTriangulation does it (src/ORBmatcher.cc:684-697, :800-810)
void intersect_feature_vectors(const DBoW2::FeatureVector &v1, const DBoW2::FeatureVector &v2, Lists &L) {
    L.sq.assign(1, 0); L.sc.assign(1, 0); L.iq.clear(); L.ic.clear();
    DBoW2::FeatureVector::const_iterator f1it = v1.begin(), f2it = v2.begin(), f1end = v1.end(), f2end = v2.end();
    while (f1it != f1end && f2it != f2end) {
        if (f1it->first == f2it->first) {
            L.iq.insert(L.iq.end(), f1it->second.begin(), f1it->second.end());
            L.ic.insert(L.ic.end(), f2it->second.begin(), f2it->second.end());
            L.sq.push_back((int32_t)L.iq.size()); L.sc.push_back((int32_t)L.ic.size());
            f1it++; f2it++;
        } else if (f1it->first < f2it->first) f1it = v1.lower_bound(f2it->first);
        else f2it = v2.lower_bound(f1it->first);
    }
}
}  // namespace

cv::Mat LocalMapping::SkewSymmetricMatrix(const cv::Mat &v) {
    cv::Mat m = cv::Mat::zeros(3, 3, CV_32F);
    m.at<float>(0, 1) = -v.at<float>(2); m.at<float>(0, 2) = v.at<float>(1);
    m.at<float>(1, 0) = v.at<float>(2); m.at<float>(1, 2) = -v.at<float>(0);
    m.at<float>(2, 0) = -v.at<float>(1); m.at<float>(2, 1) = v.at<float>(0);
    return m;
}

cv::Mat LocalMapping::ComputeF12(KeyFrame *&pKF1, KeyFrame *&pKF2) {
    float T1[16], T2[16], F[9];
    const cv::Mat P1 = pKF1->GetPose(), P2 = pKF2->GetPose();
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) { T1[r * 4 + c] = P1.at<float>(r, c); T2[r * 4 + c] = P2.at<float>(r, c); }
    const float K1[4] = {pKF1->fx, pKF1->fy, pKF1->cx, pKF1->cy}, K2[4] = {pKF2->fx, pKF2->fy, pKF2->cx, pKF2->cy};   // mK's entries
    if (orbl_compute_f12(T1, K1, T2, K2, F) != ORBX_OK) throw std::runtime_error(std::string("ComputeF12: ") + orbx_last_error());
    cv::Mat F12(3, 3, CV_32F);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) F12.at<float>(r, c) = F[r * 3 + c];
    return F12;
}

void LocalMapping::CreateNewMapPoints() {
    // Retrieve neighbor keyframes in covisibility graph (:218-221)
    int nn = 10;
    if (mbMonocular) nn = 20;
    const std::vector<KeyFrame *> vpNeighKFs = mpCurrentKeyFrame->GetBestCovisibilityKeyFrames(nn);
    const int nnb = (int)vpNeighKFs.size(), nq = mpCurrentKeyFrame->N;
    if (nnb == 0 || nq == 0) return;
    Side cur;
    cur.gather(mpCurrentKeyFrame);
    std::vector<Side> sides(nnb);
    std::vector<Lists> lists(nnb);
    std::vector<orbl_neighbour_t> nbs(nnb);
    const cv::Mat Cw = mpCurrentKeyFrame->GetCameraCenter();
    for (int i = 0; i < nnb; i++) {
        KeyFrame *pKF2 = vpNeighKFs[i];
        sides[i].gather(pKF2);
        intersect_feature_vectors(mpCurrentKeyFrame->mFeatVec, pKF2->mFeatVec, lists[i]);
        orbl_neighbour_t &b = nbs[i];
        b.kf = sides[i].kf; b.c_desc = sides[i].desc.data(); b.c_flags = sides[i].flags.data();
        b.node_qstart = lists[i].sq.data(); b.q_items = lists[i].iq.data(); b.node_cstart = lists[i].sc.data(); b.c_items = lists[i].ic.data();
        b.nnodes = (int32_t)lists[i].sq.size() - 1;
        const cv::Mat F12 = ComputeF12(mpCurrentKeyFrame, pKF2);   // :272
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) b.F12[r * 3 + c] = F12.at<float>(r, c);
        // the epipole in the second image (src/ORBmatcher.cc:663-670): C2 = R2w*Cw + t2w a gemm with an addend
        const cv::Mat T2 = pKF2->GetPose();
        float C2[3];
        for (int r = 0; r < 3; r++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += (double)T2.at<float>(r, k) * (double)Cw.at<float>(k);
            C2[r] = (float)(s + (double)T2.at<float>(r, 3));
        }
        const float invz = 1.0f / C2[2];
        b.ex = pKF2->fx * C2[0] * invz + pKF2->cx;
        b.ey = pKF2->fy * C2[1] * invz + pKF2->cy;
        b.median_depth2 = mbMonocular ? pKF2->ComputeSceneMedianDepth(2) : 0.f;   // :264
    }
    std::vector<int32_t> match((size_t)nnb * nq), nmatches(nnb), nnew(nnb);
    std::vector<orbl_point_t> points((size_t)nnb * nq);
    std::vector<uint8_t> skipped(nnb), flagsOut(nq);
    // ORBmatcher matcher(0.6,false) (:223): no orientation check; TH_LOW = 50
    if (orbl_create_new_map_points(&cur.kf, cur.desc.data(), cur.flags.data(), nbs.data(), nnb, mbMonocular ? 1 : 0, 50, 0, match.data(), points.data(),
                                   nmatches.data(), nnew.data(), skipped.data(), flagsOut.data(), device) != ORBX_OK)
        throw std::runtime_error(std::string("CreateNewMapPoints: ") + orbx_last_error());
    for (int i = 0; i < nnb; i++) {
        if (i > 0 && CheckNewKeyFrames()) return;   // :247-248
        if (skipped[i]) continue;                   // :259-268
        KeyFrame *pKF2 = vpNeighKFs[i];
        for (int idx1 = 0; idx1 < nq; idx1++) {
            const orbl_point_t &p = points[(size_t)i * nq + idx1];
            if (p.status < 0) continue;
            const int idx2 = match[(size_t)i * nq + idx1];
            // Triangulation is succesfull (:442-457)
            cv::Mat x3D(3, 1, CV_32F);
            x3D.at<float>(0) = p.x; x3D.at<float>(1) = p.y; x3D.at<float>(2) = p.z;
            MapPoint *pMP = new MapPoint(x3D, mpCurrentKeyFrame, mpMap);
            pMP->AddObservation(mpCurrentKeyFrame, idx1);
            pMP->AddObservation(pKF2, idx2);
            mpCurrentKeyFrame->AddMapPoint(pMP, idx1);
            pKF2->AddMapPoint(pMP, idx2);
            pMP->ComputeDistinctiveDescriptors();
            pMP->UpdateNormalAndDepth();
            mpMap->AddMapPoint(pMP);
            mlpRecentAddedMapPoints.push_back(pMP);
        }
    }
}

void LocalMapping::KeyFrameCulling() {
    const std::vector<KeyFrame *> vpLocalKeyFrames = mpCurrentKeyFrame->GetVectorCovisibleKeyFrames();   // :646
    if (vpLocalKeyFrames.empty()) return;
    CovisTables T;
    T.Build(vpLocalKeyFrames, std::vector<MapPoint *>());
    const size_t Q = vpLocalKeyFrames.size();
    std::vector<int32_t> nMPs(Q), nRedundant(Q), verdict(Q);
    if (orbc_keyframe_culling(&T.table, &T.queries, mbMonocular ? 1 : 0, 3, nMPs.data(), nRedundant.data(), verdict.data(), NULL, device) != ORBX_OK)
        throw std::runtime_error(std::string("KeyFrameCulling: ") + orbx_last_error());
    for (size_t q = 0; q < Q; q++)
        if (verdict[q]) vpLocalKeyFrames[q]->SetBadFlag();   // :701-702; 2: the keyframe's mbNotErase turns it into mbToBeErased
}

}  // namespace ORB_SLAM2
