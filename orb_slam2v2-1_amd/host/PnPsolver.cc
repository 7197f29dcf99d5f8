// PnPsolver.cc — see PnPsolver.h.
#include "PnPsolver.h"
#include <algorithm>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include "dutils_random.h"

namespace ORB_SLAM2 {

int PnPsolver::device = std::getenv("ORBX_DEVICE") ? std::atoi(std::getenv("ORBX_DEVICE")) : 0;

static cv::Mat toMat(const float *T) {
    cv::Mat M(4, 4, CV_32F);
    for (int k = 0; k < 16; k++) M.at<float>(k / 4, k % 4) = T[k];
    return M;
}

PnPsolver::PnPsolver(const Frame &F, const std::vector<MapPoint *> &vpMapPointMatches)
    : mnIterations(0), mnBestInliers(0), N(0), mbSetsGiven(false) {
    mvpMapPointMatches = vpMapPointMatches;
    mvCorrs.reserve(F.mvpMapPoints.size());
    mvKeyPointIndices.reserve(F.mvpMapPoints.size());

    for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {   // :79-101
        MapPoint *pMP = vpMapPointMatches[i];

        if (pMP) {
            if (!pMP->isBad()) {
                const cv::KeyPoint &kp = F.mvKeysUn[i];

                orbp_corr_t c;
                c.u = kp.pt.x; c.v = kp.pt.y;
                c.sigma2 = F.mvLevelSigma2[kp.octave];

                cv::Mat Pos = pMP->GetWorldPos();
                for (int k = 0; k < 3; k++) c.w[k] = Pos.at<float>(k);
                mvCorrs.push_back(c);

                mvKeyPointIndices.push_back(i);
            }
        }
    }

    // Set camera calibration parameters
    mK[0] = F.fx; mK[1] = F.fy; mK[2] = F.cx; mK[3] = F.cy;

    SetRansacParameters();
}

void PnPsolver::SetRansacParameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon, float th2) {
    mRansacProb = probability;
    mRansacEpsilon = epsilon;
    mRansacMinSet = minSet;
    mTh2 = th2;
    N = (int)mvCorrs.size();   // number of correspondences
    // :133-152, as host code of the library
    if (orbp_pnp_parameters(N, probability, minInliers, maxIterations, minSet, epsilon, &mRansacMinInliers, &mRansacMaxIts) != ORBX_OK)
        throw std::runtime_error(std::string("PnPsolver: ") + orbx_last_error());
}

void PnPsolver::SetSets(const std::vector<int32_t> &sets) {
    mvSets = sets;
    mbSetsGiven = true;
}

int PnPsolver::Planned(int nIterations) const {   // while(mnIterations<mRansacMaxIts || nCurrentIterations<nIterations)
    if (N < mRansacMinInliers) return 0;
    return std::max(mRansacMaxIts - mnIterations, std::max(nIterations, 0));
}

void PnPsolver::DrawSets(int its) {
    if (mbSetsGiven) {
        if (mvSets.size() < (size_t)its * 4) throw std::runtime_error("PnPsolver: fewer sets given than iterations");
        mvSets.resize((size_t)its * 4);
        mbSetsGiven = false;
        return;
    }
    // :188-201, for all iterations of the call at once
    std::vector<size_t> vAllIndices, vAvailableIndices;
    for (int i = 0; i < N; i++) vAllIndices.push_back(i);
    mvSets.assign((size_t)its * 4, 0);
    for (int it = 0; it < its; it++) {
        vAvailableIndices = vAllIndices;
        for (short i = 0; i < 4; ++i) {
            int randi = DUtils::Random::RandomInt(0, (int)vAvailableIndices.size() - 1);
            mvSets[(size_t)it * 4 + i] = (int32_t)vAvailableIndices[randi];
            vAvailableIndices[randi] = vAvailableIndices.back();
            vAvailableIndices.pop_back();
        }
    }
}

orbp_problem_t PnPsolver::Problem() const {
    orbp_problem_t p;
    for (int k = 0; k < 4; k++) p.K[k] = mK[k];
    p.th2 = mTh2;
    p.min_inliers = mRansacMinInliers;
    p.max_iterations = mRansacMaxIts;
    p.iterations_done = mnIterations;
    p.prior_best_inliers = mnBestInliers;
    return p;
}

cv::Mat PnPsolver::Absorb(const orbp_pnp_info_t &info, const uint8_t *inliers, const uint8_t *best, bool &bNoMore,
                          std::vector<bool> &vbInliers, int &nInliers) {
    mnIterations += info.iterations_run;
    mnBestInliers = info.best_inliers;
    mvbBestInliers.assign(best, best + N);
    if (info.best_iteration >= 0) mBestTcw = toMat(info.best_Tcw);
    bNoMore = info.no_more != 0;
    if (info.pose == ORBP_POSE_NONE) return cv::Mat();
    nInliers = info.pose == ORBP_POSE_REFINED ? info.refined_inliers : info.best_inliers;
    vbInliers = std::vector<bool>(mvpMapPointMatches.size(), false);
    for (int i = 0; i < N; i++)
        if (inliers[i])
            vbInliers[mvKeyPointIndices[i]] = true;
    return info.pose == ORBP_POSE_REFINED ? toMat(info.Tcw) : mBestTcw.clone();
}

void PnPsolver::IterateAll(std::vector<PnPsolver *> &vpSolvers, int nIterations, std::vector<cv::Mat> &vTcw, std::vector<bool> &vbNoMore,
                           std::vector<std::vector<bool> > &vvbInliers, std::vector<int> &vnInliers) {
    const size_t S = vpSolvers.size();
    vTcw.assign(S, cv::Mat());
    vbNoMore.assign(S, false);
    vvbInliers.assign(S, std::vector<bool>());
    vnInliers.assign(S, 0);
    std::vector<size_t> todo;
    for (size_t i = 0; i < S; i++) {
        PnPsolver *s = vpSolvers[i];
        if (!s) continue;
        if (s->N < s->mRansacMinInliers) vbNoMore[i] = true;   // :173-177
        else todo.push_back(i);
    }
    if (todo.empty()) return;
    std::vector<orbp_corr_t> corrs;
    std::vector<orbp_problem_t> problems;
    std::vector<int32_t> offsets(1, 0), setOffsets(1, 0), sets;
    std::vector<uint8_t> prior;
    for (size_t k = 0; k < todo.size(); k++) {
        PnPsolver *s = vpSolvers[todo[k]];
        s->DrawSets(s->Planned(nIterations));
        corrs.insert(corrs.end(), s->mvCorrs.begin(), s->mvCorrs.end());
        sets.insert(sets.end(), s->mvSets.begin(), s->mvSets.end());
        if (s->mvbBestInliers.empty()) prior.insert(prior.end(), (size_t)s->N, 0);
        else prior.insert(prior.end(), s->mvbBestInliers.begin(), s->mvbBestInliers.end());
        problems.push_back(s->Problem());
        offsets.push_back((int32_t)corrs.size());
        setOffsets.push_back((int32_t)(sets.size() / 4));
    }
    std::vector<int32_t> counts(sets.size() / 4 + 1);
    std::vector<uint8_t> inl(corrs.size() + 1), best(corrs.size() + 1);
    std::vector<orbp_pnp_info_t> infos(todo.size());
    sets.push_back(0);
    const int rc = orbp_pnp_ransac_batch(corrs.data(), offsets.data(), (int)todo.size(), problems.data(), sets.data(), setOffsets.data(),
                                         prior.data(), counts.data(), NULL, NULL, NULL, NULL, NULL, inl.data(), best.data(), infos.data(), device);
    if (rc != ORBX_OK) throw std::runtime_error(std::string("PnPsolver: ") + orbx_last_error());
    for (size_t k = 0; k < todo.size(); k++) {
        const size_t i = todo[k];
        bool nm = false;
        vTcw[i] = vpSolvers[i]->Absorb(infos[k], inl.data() + offsets[k], best.data() + offsets[k], nm, vvbInliers[i], vnInliers[i]);
        vbNoMore[i] = nm;
    }
}

cv::Mat PnPsolver::iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers) {
    std::vector<PnPsolver *> self(1, this);
    std::vector<cv::Mat> vTcw;
    std::vector<bool> vbNoMore;
    std::vector<std::vector<bool> > vvbInliers;
    std::vector<int> vnInliers;
    IterateAll(self, nIterations, vTcw, vbNoMore, vvbInliers, vnInliers);
    bNoMore = vbNoMore[0];
    vbInliers = vvbInliers[0];
    nInliers = vnInliers[0];
    return vTcw[0];
}

cv::Mat PnPsolver::find(std::vector<bool> &vbInliers, int &nInliers) {
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers);
}

}  // namespace ORB_SLAM2
