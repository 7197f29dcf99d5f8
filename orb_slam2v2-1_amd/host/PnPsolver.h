// PnPsolver.h — ORB_SLAM2::PnPsolver (include/PnPsolver.h, src/PnPsolver.cc) executed on an MI355X through include/orbx.h
// (orbp_pnp_ransac_batch): the EPnP RANSAC Tracking::Relocalization (src/Tracking.cc:1530-1556) runs for every candidate keyframe.
// The class keeps the reference's bookkeeping - the filtering of the matched map points, mvKeyPointIndices, SetRansacParameters,
// mnIterations / mnBestInliers / mvbBestInliers / mBestTcw from call to call - and hands every iterate() call to the library as
// ONE device call over the max(mRansacMaxIts - mnIterations, nIterations) iterations the reference's loop may run.  IterateAll
// does that for all live candidates of a Relocalization pass with one batched call.
// Unlike the reference, which draws a set when its iteration runs - so that several solvers interleave their rand() draws - a
// solver here draws all sets of a call at that call (as Sim3Solver.h states for its own).
#ifndef ORBX_PNPSOLVER_H
#define ORBX_PNPSOLVER_H
#include <cstdint>
#include <vector>
#include "frame_shim.h"
#include "orbx.h"

namespace ORB_SLAM2 {

class PnPsolver {
public:
    PnPsolver(const Frame &F, const std::vector<MapPoint *> &vpMapPointMatches);

    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4,
                             float th2 = 5.991);

    cv::Mat find(std::vector<bool> &vbInliers, int &nInliers);

    // An empty matrix, or Tcw (4x4 CV_32F) with vbInliers (one entry per element of vpMapPointMatches, indexed by keypoint) and
    // nInliers: the refined pose at a hit, the best pose when the iterations are used up (bNoMore) and the best count reaches
    // minInliers.  Throws std::runtime_error with orbx_last_error() when the library reports an error (no GPU, minSet != 4).
    cv::Mat iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers);

    // iterate(nIterations) of every solver (null entries are skipped) as ONE batched device call; the four result vectors get one
    // entry per solver
    static void IterateAll(std::vector<PnPsolver *> &vpSolvers, int nIterations, std::vector<cv::Mat> &vTcw, std::vector<bool> &vbNoMore,
                           std::vector<std::vector<bool> > &vvbInliers, std::vector<int> &vnInliers);

    // The sets of the NEXT device call, [iterations][4] indices into the accepted correspondences, instead of drawing them with
    // rand() (at least as many as the call may run; the first ones are used)
    void SetSets(const std::vector<int32_t> &sets);
    std::vector<int32_t> mvSets;                // the sets of the last call
    std::vector<size_t> mvKeyPointIndices;      // index in vpMapPointMatches of each accepted correspondence
    int mRansacMinInliers, mRansacMaxIts;
    int mnIterations, mnBestInliers;
    static int device;                          // GPU used (default: ORBX_DEVICE or 0)

private:
    int Planned(int nIterations) const;
    void DrawSets(int its);
    orbp_problem_t Problem() const;
    cv::Mat Absorb(const orbp_pnp_info_t &info, const uint8_t *inliers, const uint8_t *best, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers);

    std::vector<MapPoint *> mvpMapPointMatches;
    std::vector<orbp_corr_t> mvCorrs;           // world position, keypoint and sigma2 of the accepted correspondences
    int N;
    float mK[4], mTh2;
    bool mbSetsGiven;
    std::vector<uint8_t> mvbBestInliers;
    cv::Mat mBestTcw;
    double mRansacProb;
    float mRansacEpsilon;
    int mRansacMinSet;
};

}  // namespace ORB_SLAM2
#endif
