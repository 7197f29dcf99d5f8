// localmap_driver.cc — ORB_SLAM2::Tracking::UpdateLocalMap / SearchLocalPoints and LocalMapHIP (orb_slam2v2-1_amd/host/Tracking.h) on
// shim objects built from a scene blob, for tests/test_localmap_host_cpp_gpu.py.
//   localmap_driver IN
//   IN: the blob of tests/cpp/localmap_lockstep.cc, then int32 has_frame and, if set: float fx fy cx cy mbf mb minx miny maxx maxy log_sf |
//       float Tcw[16] | int32 sensor frame_id last_reloc_id | orbx_keypoint_t[N] | uint8 desc[N][32] | float uright[N]
//   prints: "info <empty_vote> <n_voted> <ref keyframe or -1> <extension_end>", "kf ..." (mvpLocalKeyFrames), "pts ..." (mvpLocalMapPoints),
//           "frame ..." (mCurrentFrame.mvpMapPoints, -1 for NULL), "kfmarks ..." / "ptmarks ..." (the objects whose mnTrackReferenceForFrame
//           is the frame's id), "ref <mpReferenceKF> <mCurrentFrame.mpReferenceKF>"; with a frame also "search <matches> <nToMatch>
//           <matches of the old way> <its nToMatch> <same>": Tracking::SearchLocalPoints on one world, the reference's first loop +
//           SearchLocalPointsHIP with the same lists on a copy of it, and whether every frame slot and every point's tracking
//           members are equal, then "frame2 ..." (the slots after the search)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "ORBmatcher.h"
#include "Tracking.h"

using namespace ORB_SLAM2;

template <typename T> static bool rd(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n + 1);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

struct Blob {
    int32_t hd[11];
    std::vector<orbc_keyframe_t> kf;
    std::vector<orbc_point_t> pts;
    std::vector<int32_t> off, foff, parent, coff, cov, hoff, child, fpts, prev;
    std::vector<orbc_observation_t> obs;
    std::vector<float> sf, uright;
    std::vector<orbc_feature_t> feat;
    std::vector<orbt_pointview_t> views;
    std::vector<uint8_t> desc, fdesc;
    int32_t has_frame, ids[3];
    float cam[11], Tcw[16];
    std::vector<orbx_keypoint_t> kp;
};

static bool read_blob(const char *path, Blob &b) {
    FILE *f = fopen(path, "rb");
    if (!f || fread(b.hd, 4, 11, f) != 11) return false;
    const int K = b.hd[0], P = b.hd[1], N = b.hd[7];
    if (!rd(f, b.kf, K) || !rd(f, b.pts, P) || !rd(f, b.off, P + 1) || !rd(f, b.obs, b.hd[2]) || !rd(f, b.sf, b.hd[3]) || !rd(f, b.foff, K + 1) ||
        !rd(f, b.feat, b.hd[4]) || !rd(f, b.parent, K) || !rd(f, b.coff, K + 1) || !rd(f, b.cov, b.hd[5]) || !rd(f, b.hoff, K + 1) || !rd(f, b.child, b.hd[6]) ||
        !rd(f, b.views, P) || !rd(f, b.desc, (size_t)P * 32) || !rd(f, b.fpts, N) || !rd(f, b.prev, b.hd[8])) return false;
    if (fread(&b.has_frame, 4, 1, f) != 1) return false;
    if (b.has_frame && (fread(b.cam, 4, 11, f) != 11 || fread(b.Tcw, 4, 16, f) != 16 || fread(b.ids, 4, 3, f) != 3 || !rd(f, b.kp, N) || !rd(f, b.fdesc, (size_t)N * 32) ||
                        !rd(f, b.uright, N))) return false;
    fclose(f);
    return true;
}

struct World {
    std::vector<KeyFrame> kfs;
    std::vector<MapPoint> mps;
    Map map;
    Tracking tr;
    void build(const Blob &b) {
        const int K = b.hd[0], P = b.hd[1], N = b.hd[7];
        kfs.resize(K); mps.resize(P);
        for (int p = 0; p < P; p++) {
            MapPoint &m = mps[p];
            m.mbBad = b.pts[p].bad != 0; m.nObs = b.views[p].observations; m.mfMaxDistance = b.views[p].max_distance; m.mfMinDistance = b.views[p].min_distance;
            for (int c = 0; c < 3; c++) { m.mWorldPos.at<float>(c) = b.pts[p].pos[c]; m.mNormalVector.at<float>(c) = b.views[p].normal[c]; }
            m.mDescriptor = cv::Mat(1, 32, CV_8U);
            memcpy(m.mDescriptor.ptr(0), &b.desc[(size_t)32 * p], 32);
            for (int o = b.off[p]; o < b.off[p + 1]; o++) m.mObservations[&kfs[b.obs[o].kf]] = (size_t)b.obs[o].idx;
            map.AddMapPoint(&m);
        }
        for (int s = 0; s < K; s++) {
            KeyFrame &k = kfs[s];
            k.mnId = (long unsigned int)b.kf[s].id; k.mbBad = b.kf[s].bad != 0; k.mvScaleFactors = std::vector<float>(b.sf.begin(), b.sf.begin() + b.hd[3]);
            k.N = b.foff[s + 1] - b.foff[s];
            for (int f = b.foff[s]; f < b.foff[s + 1]; f++) k.mvpMapPoints.push_back(b.feat[f].point >= 0 ? &mps[b.feat[f].point] : static_cast<MapPoint *>(NULL));
            if (b.parent[s] >= 0) k.mpParent = &kfs[b.parent[s]];
            for (int c = b.coff[s]; c < b.coff[s + 1]; c++) k.mvpOrderedConnectedKeyFrames.push_back(&kfs[b.cov[c]]);
            for (int c = b.hoff[s]; c < b.hoff[s + 1]; c++) k.mspChildrens.insert(&kfs[b.child[c]]);
            map.AddKeyFrame(&k);
        }
        tr.mpMap = &map;
        Frame &F = tr.mCurrentFrame;
        F.N = N; F.mnId = 7;
        for (int i = 0; i < N; i++) F.mvpMapPoints.push_back(b.fpts[i] >= 0 ? &mps[b.fpts[i]] : static_cast<MapPoint *>(NULL));
        for (int j = 0; j < b.hd[8]; j++) tr.mvpLocalKeyFrames.push_back(&kfs[b.prev[j]]);
        if (!b.has_frame) return;
        Frame::fx = b.cam[0]; Frame::fy = b.cam[1]; Frame::cx = b.cam[2]; Frame::cy = b.cam[3]; F.mbf = b.cam[4]; F.mb = b.cam[5];
        Frame::mnMinX = b.cam[6]; Frame::mnMinY = b.cam[7]; Frame::mnMaxX = b.cam[8]; Frame::mnMaxY = b.cam[9];
        Frame::mfGridElementWidthInv = 64.f / (Frame::mnMaxX - Frame::mnMinX); Frame::mfGridElementHeightInv = 48.f / (Frame::mnMaxY - Frame::mnMinY);
        F.mfLogScaleFactor = b.cam[10]; F.mnScaleLevels = b.hd[3]; F.mvScaleFactors = std::vector<float>(b.sf.begin(), b.sf.begin() + b.hd[3]);
        F.mTcw = cv::Mat(4, 4, CV_32F);
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) F.mTcw.at<float>(r, c) = b.Tcw[r * 4 + c];
        tr.mSensor = b.ids[0]; F.mnId = (long unsigned int)b.ids[1]; tr.mnLastRelocFrameId = (unsigned int)b.ids[2];
        F.mvKeysUn.resize(N); F.mvuRight.assign(b.uright.begin(), b.uright.begin() + N);
        F.mDescriptors = cv::Mat(N, 32, CV_8U);
        for (int i = 0; i < N; i++) {
            cv::KeyPoint &k = F.mvKeysUn[i];
            k.pt.x = b.kp[i].x; k.pt.y = b.kp[i].y; k.size = b.kp[i].size; k.angle = b.kp[i].angle; k.response = b.kp[i].response; k.octave = b.kp[i].octave;
            k.class_id = b.kp[i].class_id;
            memcpy(F.mDescriptors.ptr(i), &b.fdesc[(size_t)32 * i], 32);
        }
        F.mvKeys = F.mvKeysUn;
    }
};

static void print_slots(const char *tag, const World &w, const std::vector<MapPoint *> &v) {
    printf("%s", tag);
    for (size_t i = 0; i < v.size(); i++) printf(" %d", v[i] ? (int)(v[i] - &w.mps[0]) : -1);
    printf("\n");
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: localmap_driver IN\n"); return 2; }
    static Blob b;
    if (!read_blob(argv[1], b)) { fprintf(stderr, "localmap_driver: short blob\n"); return 1; }
    static World A, B;
    A.build(b);
    try {
        Tracking &t = A.tr;
        t.mLocalMap.Rebuild(&A.map);
        t.UpdateLocalMap();
        const long unsigned int id = t.mCurrentFrame.mnId;
        printf("info %d %d %d %d\n", t.mLocalInfo.empty_vote, t.mLocalInfo.n_voted, t.mLocalInfo.ref_kf, t.mLocalInfo.extension_end);
        printf("kf");
        for (size_t j = 0; j < t.mvpLocalKeyFrames.size(); j++) printf(" %d", (int)(t.mvpLocalKeyFrames[j] - &A.kfs[0]));
        printf("\n");
        print_slots("pts", A, t.mvpLocalMapPoints);
        print_slots("frame", A, t.mCurrentFrame.mvpMapPoints);
        printf("kfmarks");
        for (size_t s = 0; s < A.kfs.size(); s++) if (A.kfs[s].mnTrackReferenceForFrame == id) printf(" %d", (int)s);
        printf("\nptmarks");
        for (size_t p = 0; p < A.mps.size(); p++) if (A.mps[p].mnTrackReferenceForFrame == id) printf(" %d", (int)p);
        printf("\nref %d %d\n", t.mpReferenceKF ? (int)(t.mpReferenceKF - &A.kfs[0]) : -1,
               t.mCurrentFrame.mpReferenceKF ? (int)(t.mCurrentFrame.mpReferenceKF - &A.kfs[0]) : -1);
        if (!b.has_frame) return 0;
        // the old way on a copy of the world: the same lists, the reference's first loop (src/Tracking.cc:1291-1307), then SearchLocalPointsHIP
        B.build(b);
        Frame &FB = B.tr.mCurrentFrame;
        std::vector<MapPoint *> localB;
        for (size_t j = 0; j < t.mvpLocalMapPoints.size(); j++) localB.push_back(&B.mps[t.mvpLocalMapPoints[j] - &A.mps[0]]);
        for (size_t i = 0; i < FB.mvpMapPoints.size(); i++) {
            MapPoint *pMP = FB.mvpMapPoints[i];
            if (!pMP) continue;
            if (pMP->isBad()) FB.mvpMapPoints[i] = static_cast<MapPoint *>(NULL);
            else { pMP->IncreaseVisible(); pMP->mnLastFrameSeen = FB.mnId; pMP->mbTrackInView = false; }
        }
        int th = 1;
        if (B.tr.mSensor == System::RGBD) th = 3;
        if (FB.mnId < B.tr.mnLastRelocFrameId + 2) th = 5;
        int nToMatchB = 0;
        const int nB = SearchLocalPointsHIP(FB, localB, (float)th, 0.8f, nToMatchB);
        t.SearchLocalPoints();
        bool same = t.mCurrentFrame.mvpMapPoints.size() == FB.mvpMapPoints.size();
        for (size_t i = 0; same && i < FB.mvpMapPoints.size(); i++) {
            MapPoint *a = t.mCurrentFrame.mvpMapPoints[i], *c = FB.mvpMapPoints[i];
            same = (a == NULL) == (c == NULL) && (!a || a - &A.mps[0] == c - &B.mps[0]);
        }
        for (size_t p = 0; same && p < A.mps.size(); p++) {
            const MapPoint &a = A.mps[p], &c = B.mps[p];
            same = a.mbTrackInView == c.mbTrackInView && a.mnVisible == c.mnVisible && a.mnLastFrameSeen == c.mnLastFrameSeen && a.mnTrackScaleLevel == c.mnTrackScaleLevel &&
                   !memcmp(&a.mTrackProjX, &c.mTrackProjX, 4) && !memcmp(&a.mTrackProjXR, &c.mTrackProjXR, 4) && !memcmp(&a.mTrackProjY, &c.mTrackProjY, 4) &&
                   !memcmp(&a.mTrackViewCos, &c.mTrackViewCos, 4);
        }
        printf("search %d %d %d %d %d\n", t.mnMatchesLocal, t.mnToMatch, nB, nToMatchB, (int)same);
        print_slots("frame2", A, t.mCurrentFrame.mvpMapPoints);
    } catch (const std::exception &e) {
        fprintf(stderr, "localmap_driver: %s\n", e.what());
        return 1;
    }
    return 0;
}
