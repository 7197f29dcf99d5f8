// Initializer.cc — see Initializer.h.
#include "Initializer.h"
#include <cstdlib>
#include <stdexcept>
#include <string>
#include "dutils_random.h"
#include "orbx.h"

namespace ORB_SLAM2 {

int Initializer::device = std::getenv("ORBX_DEVICE") ? std::atoi(std::getenv("ORBX_DEVICE")) : 0;

Initializer::Initializer(const Frame &ReferenceFrame, float sigma, int iterations) {
    mK = ReferenceFrame.mK.clone();
    mvKeys1 = ReferenceFrame.mvKeysUn;
    mSigma = sigma;
    mSigma2 = sigma * sigma;
    mMaxIterations = iterations;
}

bool Initializer::Initialize(const Frame &CurrentFrame, const std::vector<int> &vMatches12, cv::Mat &R21, cv::Mat &t21,
                             std::vector<cv::Point3f> &vP3D, std::vector<bool> &vbTriangulated) {
    // Reference Frame: 1, Current Frame: 2 (:49-63)
    mvKeys2 = CurrentFrame.mvKeysUn;
    mvMatches12.clear();
    mvMatches12.reserve(mvKeys2.size());
    mvbMatched1.resize(mvKeys1.size());
    for (size_t i = 0, iend = vMatches12.size(); i < iend; i++) {
        if (vMatches12[i] >= 0) {
            mvMatches12.push_back(std::make_pair((int)i, vMatches12[i]));
            mvbMatched1[i] = true;
        } else
            mvbMatched1[i] = false;
    }
    const int N = (int)mvMatches12.size();
    if (N < 8) throw std::runtime_error("Initializer::Initialize: fewer than 8 matches");

    // Generate sets of 8 points for each RANSAC iteration (:67-97)
    std::vector<size_t> vAllIndices, vAvailableIndices;
    vAllIndices.reserve(N);
    for (int i = 0; i < N; i++) vAllIndices.push_back(i);
    mvSets = std::vector<std::vector<size_t> >(mMaxIterations, std::vector<size_t>(8, 0));
    DUtils::Random::SeedRandOnce(0);
    for (int it = 0; it < mMaxIterations; it++) {
        vAvailableIndices = vAllIndices;
        for (size_t j = 0; j < 8; j++) {
            int randi = DUtils::Random::RandomInt(0, (int)vAvailableIndices.size() - 1);
            int idx = (int)vAvailableIndices[randi];
            mvSets[it][j] = idx;
            vAvailableIndices[randi] = vAvailableIndices.back();
            vAvailableIndices.pop_back();
        }
    }

    std::vector<float> k1(mvKeys1.size() * 2), k2(mvKeys2.size() * 2), P3D((size_t)N * 3);
    for (size_t i = 0; i < mvKeys1.size(); i++) { k1[2 * i] = mvKeys1[i].pt.x; k1[2 * i + 1] = mvKeys1[i].pt.y; }
    for (size_t i = 0; i < mvKeys2.size(); i++) { k2[2 * i] = mvKeys2[i].pt.x; k2[2 * i + 1] = mvKeys2[i].pt.y; }
    std::vector<int32_t> matches((size_t)N * 2), sets((size_t)mMaxIterations * 8);
    for (int i = 0; i < N; i++) { matches[2 * i] = mvMatches12[i].first; matches[2 * i + 1] = mvMatches12[i].second; }
    for (int it = 0; it < mMaxIterations; it++)
        for (int j = 0; j < 8; j++) sets[it * 8 + j] = (int32_t)mvSets[it][j];
    std::vector<uint8_t> tri(N);
    const float K4[4] = {mK.at<float>(0, 0), mK.at<float>(1, 1), mK.at<float>(0, 2), mK.at<float>(1, 2)};
    float R[9], t[3];
    int result = 0;
    orbi_init_info_t info;
    // ReconstructH / ReconstructF are called with minParallax 1.0 and minTriangulated 50 (:116, :118)
    const int rc = orbi_initialize(k1.data(), (int)mvKeys1.size(), k2.data(), (int)mvKeys2.size(), matches.data(), N, sets.data(),
                                   mMaxIterations, K4, mSigma, 1.0f, 50, &result, R, t, P3D.data(), tri.data(), &info, device);
    if (rc != ORBX_OK) throw std::runtime_error(std::string("Initializer::Initialize: ") + orbx_last_error());
    if (!result) {
        if (info.model == 1 && info.best_iteration[1] >= 0) { R21 = cv::Mat(); t21 = cv::Mat(); }
        return false;
    }
    R21 = cv::Mat(3, 3, CV_32F);
    t21 = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) R21.at<float>(r, c) = R[r * 3 + c];
        t21.at<float>(r) = t[r];
    }
    // CheckRT sizes both by the reference keypoints and indexes them by the match's first (:808-809, :889-893)
    vP3D.assign(mvKeys1.size(), cv::Point3f());
    vbTriangulated.assign(mvKeys1.size(), false);
    for (int i = 0; i < N; i++) {
        vP3D[mvMatches12[i].first] = cv::Point3f(P3D[3 * i], P3D[3 * i + 1], P3D[3 * i + 2]);
        vbTriangulated[mvMatches12[i].first] = tri[i] != 0;
    }
    return true;
}

}  // namespace ORB_SLAM2
