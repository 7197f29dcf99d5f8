// Sim3Solver.cc — see Sim3Solver.h.
#include "Sim3Solver.h"
#include <cstdlib>
#include <stdexcept>
#include <string>
#include "dutils_random.h"

namespace ORB_SLAM2 {

int Sim3Solver::device = std::getenv("ORBX_DEVICE") ? std::atoi(std::getenv("ORBX_DEVICE")) : 0;

Sim3Solver::Sim3Solver(KeyFrame *pKF1, KeyFrame *pKF2, const std::vector<MapPoint *> &vpMatched12, const bool bFixScale)
    : mbPrimed(false), mbSetsGiven(false), mnIterations(0), mnBestInliers(0), mBestScale(0.f), mbFixScale(bFixScale) {
    mpKF1 = pKF1;
    mpKF2 = pKF2;

    std::vector<MapPoint *> vpKeyFrameMP1 = pKF1->GetMapPointMatches();

    mN1 = (int)vpMatched12.size();

    mvpMapPoints1.reserve(mN1);
    mvpMapPoints2.reserve(mN1);
    mvpMatches12 = vpMatched12;
    mvnIndices1.reserve(mN1);
    mvPairs.reserve(mN1);

    cv::Mat Tcw1 = pKF1->GetPose(), Tcw2 = pKF2->GetPose();
    for (int k = 0; k < 16; k++) { mTcw1[k] = Tcw1.at<float>(k / 4, k % 4); mTcw2[k] = Tcw2.at<float>(k / 4, k % 4); }

    for (int i1 = 0; i1 < mN1; i1++) {   // :62-103
        if (vpMatched12[i1]) {
            MapPoint *pMP1 = vpKeyFrameMP1[i1];
            MapPoint *pMP2 = vpMatched12[i1];

            if (!pMP1)
                continue;

            if (pMP1->isBad() || pMP2->isBad())
                continue;

            int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1);
            int indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);

            if (indexKF1 < 0 || indexKF2 < 0)
                continue;

            const cv::KeyPoint &kp1 = pKF1->mvKeysUn[indexKF1];
            const cv::KeyPoint &kp2 = pKF2->mvKeysUn[indexKF2];

            orbs_pair_t p;
            p.sigma2_1 = pKF1->mvLevelSigma2[kp1.octave];
            p.sigma2_2 = pKF2->mvLevelSigma2[kp2.octave];
            cv::Mat X3D1w = pMP1->GetWorldPos(), X3D2w = pMP2->GetWorldPos();
            for (int k = 0; k < 3; k++) { p.w1[k] = X3D1w.at<float>(k); p.w2[k] = X3D2w.at<float>(k); }
            mvPairs.push_back(p);

            mvpMapPoints1.push_back(pMP1);
            mvpMapPoints2.push_back(pMP2);
            mvnIndices1.push_back(i1);
        }
    }

    // the shim's KeyFrame keeps fx, fy, cx, cy and no mK
    mK1[0] = pKF1->fx; mK1[1] = pKF1->fy; mK1[2] = pKF1->cx; mK1[3] = pKF1->cy;
    mK2[0] = pKF2->fx; mK2[1] = pKF2->fy; mK2[2] = pKF2->cx; mK2[3] = pKF2->cy;

    SetRansacParameters();
}

void Sim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations) {
    mRansacProb = probability;
    mRansacMinInliers = minInliers;
    N = (int)mvPairs.size();   // number of correspondences
    // :125-135, as host code of the library; 0 when N < minInliers, where iterate answers bNoMore without looking
    mRansacMaxIts = orbs_sim3_iterations(N, probability, minInliers, maxIterations);
    mnIterations = 0;
    mbPrimed = false;
    if (!mbSetsGiven) mvSets.clear();
}

void Sim3Solver::SetSets(const std::vector<int32_t> &sets) {
    mvSets = sets;
    mbSetsGiven = true;
    mbPrimed = false;
}

void Sim3Solver::DrawSets() {
    if (mbSetsGiven) {
        if (mvSets.size() < (size_t)mRansacMaxIts * 3) throw std::runtime_error("Sim3Solver: fewer sets given than iterations");
        return;
    }
    // :163-177, for all iterations at once
    std::vector<size_t> vAllIndices, vAvailableIndices;
    for (int i = 0; i < N; i++) vAllIndices.push_back(i);
    mvSets.assign((size_t)mRansacMaxIts * 3, 0);
    for (int it = 0; it < mRansacMaxIts; it++) {
        vAvailableIndices = vAllIndices;
        for (short i = 0; i < 3; ++i) {
            int randi = DUtils::Random::RandomInt(0, (int)vAvailableIndices.size() - 1);
            mvSets[(size_t)it * 3 + i] = (int32_t)vAvailableIndices[randi];
            vAvailableIndices[randi] = vAvailableIndices.back();
            vAvailableIndices.pop_back();
        }
    }
}

orbs_problem_t Sim3Solver::Problem() const {
    orbs_problem_t p;
    for (int k = 0; k < 16; k++) { p.Tcw1[k] = mTcw1[k]; p.Tcw2[k] = mTcw2[k]; }
    for (int k = 0; k < 4; k++) { p.K1[k] = mK1[k]; p.K2[k] = mK2[k]; }
    p.fix_scale = mbFixScale ? 1 : 0;
    p.min_inliers = mRansacMinInliers;
    return p;
}

void Sim3Solver::Store(const int32_t *counts, const float *models, const uint8_t *flags) {
    mvCounts.assign(counts, counts + mRansacMaxIts);
    mvModels.assign(models, models + (size_t)mRansacMaxIts * 13);
    mvFlags.assign(flags, flags + (size_t)mRansacMaxIts * N);
    mbPrimed = true;
}

void Sim3Solver::IterateAll(std::vector<Sim3Solver *> &vpSolvers) {
    std::vector<Sim3Solver *> todo;
    for (size_t i = 0; i < vpSolvers.size(); i++) {
        Sim3Solver *s = vpSolvers[i];
        if (s && !s->mbPrimed && s->N >= s->mRansacMinInliers && s->mRansacMaxIts > 0) todo.push_back(s);
    }
    if (todo.empty()) return;
    std::vector<orbs_pair_t> pairs;
    std::vector<orbs_problem_t> problems;
    std::vector<int32_t> offsets(1, 0), setOffsets(1, 0), sets;
    size_t nflags = 0;
    for (size_t i = 0; i < todo.size(); i++) {
        Sim3Solver *s = todo[i];
        s->DrawSets();
        pairs.insert(pairs.end(), s->mvPairs.begin(), s->mvPairs.end());
        sets.insert(sets.end(), s->mvSets.begin(), s->mvSets.begin() + (size_t)s->mRansacMaxIts * 3);
        problems.push_back(s->Problem());
        offsets.push_back((int32_t)pairs.size());
        setOffsets.push_back((int32_t)(sets.size() / 3));
        nflags += (size_t)s->mRansacMaxIts * s->N;
    }
    std::vector<int32_t> counts(sets.size() / 3);
    std::vector<float> models(sets.size() / 3 * 13);
    std::vector<uint8_t> flags(nflags + 1), hit(pairs.size() + 1);
    std::vector<orbs_sim3_info_t> infos(todo.size());
    const int rc = orbs_sim3_ransac_batch(pairs.data(), offsets.data(), (int)todo.size(), problems.data(), sets.data(), setOffsets.data(),
                                          counts.data(), models.data(), flags.data(), hit.data(), infos.data(), device);
    if (rc != ORBX_OK) throw std::runtime_error(std::string("Sim3Solver: ") + orbx_last_error());
    size_t fb = 0;
    for (size_t i = 0; i < todo.size(); i++) {
        Sim3Solver *s = todo[i];
        s->Store(counts.data() + setOffsets[i], models.data() + (size_t)setOffsets[i] * 13, flags.data() + fb);
        fb += (size_t)s->mRansacMaxIts * s->N;
    }
}

cv::Mat Sim3Solver::iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers) {
    bNoMore = false;
    vbInliers = std::vector<bool>(mN1, false);
    nInliers = 0;

    if (N < mRansacMinInliers) {
        bNoMore = true;
        return cv::Mat();
    }

    if (!mbPrimed) {
        std::vector<Sim3Solver *> self(1, this);
        IterateAll(self);
    }

    int nCurrentIterations = 0;
    while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
        nCurrentIterations++;
        const int it = mnIterations;
        mnIterations++;

        const int mnInliersi = mvCounts[it];
        if (mnInliersi >= mnBestInliers) {
            const float *m = mvModels.data() + (size_t)it * 13;
            mnBestInliers = mnInliersi;
            mBestScale = m[0];
            mBestRotation = cv::Mat(3, 3, CV_32F);
            mBestTranslation = cv::Mat(3, 1, CV_32F);
            mBestT12 = cv::Mat::eye(4, 4, CV_32F);
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) {
                    mBestRotation.at<float>(r, c) = m[1 + r * 3 + c];
                    mBestT12.at<float>(r, c) = (float)((double)m[1 + r * 3 + c] * (double)m[0]);   // sR = ms12i*mR12i
                }
                mBestTranslation.at<float>(r) = m[10 + r];
                mBestT12.at<float>(r, 3) = m[10 + r];
            }

            if (mnInliersi > mRansacMinInliers) {
                nInliers = mnInliersi;
                const uint8_t *f = mvFlags.data() + (size_t)it * N;
                for (int i = 0; i < N; i++)
                    if (f[i])
                        vbInliers[mvnIndices1[i]] = true;
                return mBestT12;
            }
        }
    }

    if (mnIterations >= mRansacMaxIts)
        bNoMore = true;

    return cv::Mat();
}

cv::Mat Sim3Solver::find(std::vector<bool> &vbInliers12, int &nInliers) {
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
}

cv::Mat Sim3Solver::GetEstimatedRotation() { return mBestRotation.clone(); }

cv::Mat Sim3Solver::GetEstimatedTranslation() { return mBestTranslation.clone(); }

float Sim3Solver::GetEstimatedScale() { return mBestScale; }

}  // namespace ORB_SLAM2
