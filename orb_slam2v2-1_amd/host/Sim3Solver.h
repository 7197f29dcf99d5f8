// Sim3Solver.h — ORB_SLAM2::Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc) executed on an MI355X through include/orbx.h
// (orbs_sim3_ransac_batch): the similarity transform LoopClosing::ComputeSim3 (src/LoopClosing.cc:248-339) looks for between the
// current keyframe and a loop candidate.  The class keeps the reference's bookkeeping - the filtering of the matched map points,
// mvnIndices1, the sets drawn with rand(), mnIterations / mnBestInliers and the early return of iterate - and hands the
// arithmetic to the library: the first iterate after SetRansacParameters draws ALL mRansacMaxIts sets, runs ONE device call and
// stores every hypothesis' count, model and flags; every iterate(k) then advances over the stored results.  IterateAll primes the
// solvers of all candidates with one batched call (before the round-robin loop of src/LoopClosing.cc:300-345).
// Unlike the reference, which draws a set when its iteration runs - so that several solvers interleave their rand() draws - a
// solver here draws all of its sets at once.
#ifndef ORBX_SIM3SOLVER_H
#define ORBX_SIM3SOLVER_H
#include <cstdint>
#include <vector>
#include "frame_shim.h"
#include "orbx.h"

namespace ORB_SLAM2 {

class Sim3Solver {
public:
    Sim3Solver(KeyFrame *pKF1, KeyFrame *pKF2, const std::vector<MapPoint *> &vpMatched12, const bool bFixScale = true);

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300);

    cv::Mat find(std::vector<bool> &vbInliers12, int &nInliers);

    // An empty matrix when no iteration of this call has more than minInliers inliers; else T12 (4x4 CV_32F), vbInliers (one entry
    // per element of vpMatched12) and nInliers.  bNoMore: all mRansacMaxIts iterations are used up, or there are fewer
    // correspondences than minInliers.  Throws std::runtime_error with orbx_last_error() when the library reports an error (no GPU).
    cv::Mat iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers);

    cv::Mat GetEstimatedRotation();
    cv::Mat GetEstimatedTranslation();
    float GetEstimatedScale();

    // One batched device call for every solver that has not run its own yet (and has at least minInliers correspondences)
    static void IterateAll(std::vector<Sim3Solver *> &vpSolvers);

    // The sets of the device call, [mRansacMaxIts][3] indices into the accepted correspondences: drawn with rand() at the first
    // iterate, or given here before it (at least mRansacMaxIts sets; the first mRansacMaxIts are used)
    void SetSets(const std::vector<int32_t> &sets);
    std::vector<int32_t> mvSets;
    std::vector<size_t> mvnIndices1;            // index in vpMatched12 of each accepted correspondence
    int mRansacMaxIts;
    static int device;                          // GPU used (default: ORBX_DEVICE or 0)

private:
    void DrawSets();
    void Store(const int32_t *counts, const float *models, const uint8_t *flags);
    orbs_problem_t Problem() const;

    KeyFrame *mpKF1, *mpKF2;
    std::vector<orbs_pair_t> mvPairs;           // world positions and sigma2 of the accepted correspondences
    std::vector<MapPoint *> mvpMapPoints1, mvpMapPoints2, mvpMatches12;
    int N, mN1;
    float mTcw1[16], mTcw2[16], mK1[4], mK2[4];

    // the device call's results
    bool mbPrimed, mbSetsGiven;
    std::vector<int32_t> mvCounts;
    std::vector<float> mvModels;                // [mRansacMaxIts][13]: s, R, t
    std::vector<uint8_t> mvFlags;               // [mRansacMaxIts][N]

    int mnIterations, mnBestInliers;
    cv::Mat mBestT12, mBestRotation, mBestTranslation;
    float mBestScale;
    bool mbFixScale;
    double mRansacProb;
    int mRansacMinInliers;
};

}  // namespace ORB_SLAM2
#endif
