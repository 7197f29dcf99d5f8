// Initializer.h — ORB_SLAM2::Initializer (include/Initializer.h, src/Initializer.cc) executed on an MI355X through include/orbx.h
// (orbi_initialize): the monocular map initialisation Tracking runs on the matches of ORBmatcher::SearchForInitialization
// (src/Tracking.cc:723, :757).  The class keeps the reference's bookkeeping - mvMatches12, mvbMatched1, the RANSAC sets drawn with
// rand() (dutils_random.h, shared with Sim3Solver.h) - and hands the arithmetic to the library.  PnPsolver is not part of this library.
#ifndef ORBX_INITIALIZER_H
#define ORBX_INITIALIZER_H
#include <utility>
#include <vector>
#include "frame_shim.h"

namespace ORB_SLAM2 {

class Initializer {
    typedef std::pair<int, int> Match;

public:
    // Fix the reference frame
    Initializer(const Frame &ReferenceFrame, float sigma = 1.0, int iterations = 200);

    // Computes in parallel a fundamental matrix and a homography, selects a model and recovers the motion and the structure.
    // vMatches12[i] = index in CurrentFrame of reference keypoint i, or < 0.  On true: R21 (3x3), t21 (3x1) CV_32F, vP3D and
    // vbTriangulated with one entry per reference keypoint.  On false: vP3D / vbTriangulated untouched; R21 / t21 untouched when
    // the homography was reconstructed, released (cv::Mat()) when the fundamental matrix was (:501-502).
    // Throws std::runtime_error with orbx_last_error() when the library reports an error (fewer than 8 matches, no GPU).
    bool Initialize(const Frame &CurrentFrame, const std::vector<int> &vMatches12, cv::Mat &R21, cv::Mat &t21,
                    std::vector<cv::Point3f> &vP3D, std::vector<bool> &vbTriangulated);

    std::vector<std::vector<size_t> > mvSets;   // the sets of the last call (the reference keeps them private)
    static int device;                          // GPU used (default: ORBX_DEVICE or 0)

private:
    std::vector<cv::KeyPoint> mvKeys1, mvKeys2;
    std::vector<Match> mvMatches12;
    std::vector<bool> mvbMatched1;
    cv::Mat mK;
    float mSigma, mSigma2;
    int mMaxIterations;
};

}  // namespace ORB_SLAM2
#endif
