// PointCloudMapping.h — the reference's dense map (include/pointcloudmapping.h, src/pointcloudmapping.cc:29-34, 83-127, 198-278) on
// an MI355X through include/orbx.h: generatePointCloud of an RGB-D keyframe, the pcl::VoxelGrid filter saveOctomap puts it through,
// and what saveOctomap makes of the accumulated map: the axis swap, octomap::OcTree insertion and the .bt file of writeBinary.
// Plane segmentation (its result is printed and never used) and PCD input / output (:139-185) stay with the caller, and so does the
// pose: Twc16 is what the reference computes with its own Eigen,
//     Eigen::Isometry3d T = ORB_SLAM2::Converter::toSE3Quat(kf->GetPose());  Eigen::Matrix4d Twc = T.inverse().matrix();
// handed over row-major (Twc16[4 * i + j] = Twc(i, j)).
#ifndef POINTCLOUDMAPPING_HIP_H
#define POINTCLOUDMAPPING_HIP_H

#include <stdint.h>
#include <vector>
#include "cv_shim.h"
#include "orbx.h"

class PointCloudMappingHIP {
public:
    typedef orbx_cloud_point_t PointT;   // pcl::PointXYZRGBA's x y z b g r a, 16 bytes
    typedef std::vector<PointT> PointCloud;

    // PointCloudMapping(resolution_): voxel.setLeafSize(resolution, resolution, resolution); a resolution <= 0 keeps the
    // reference's default 0.1.  GPU: ORBX_DEVICE or 0.  ok() tells whether the mapper exists (the reason on stderr otherwise).
    explicit PointCloudMappingHIP(double resolution_);
    ~PointCloudMappingHIP();
    bool ok() const { return mpMapper != nullptr; }
    orbx_cloudmapper_t *handle() const { return mpMapper; }

    // generatePointCloud(kf, color, depth) with kf->fx / fy / cx / cy and the inverse pose passed in.  color: CV_8UC3 / CV_8UC4 (bytes
    // 0 1 2 of a pixel become b g r); depth: CV_32F as Tracking keeps mImDepth, or the raw CV_16U with mDepthMapFactor set below.
    // Returns the unfiltered cloud in scan order (empty on error).
    PointCloud generatePointCloud(float fx, float fy, float cx, float cy, const double *Twc16, const cv::Mat &color, const cv::Mat &depth);

    // One keyframe as saveOctomap treats it: generatePointCloud, voxel.filter, *globalMap += *tmp.  Returns the number of points
    // appended (< 0: error, globalMap unchanged).
    int insertKeyFrame(float fx, float fy, float cx, float cy, const double *Twc16, const cv::Mat &color, const cv::Mat &depth);

    // The tail of saveOctomap (:198-278) on globalMap: transformPointCloud with the axis swap, OcTree tree(octree_resolution) (the
    // reference: 0.1), updateNode per point, writeBinary(oct_name).  Returns the tree's size() after pruning (0: an empty map, the
    // file is the header alone), < 0 on error (nothing is written then).
    long long saveOctomap(const char *oct_name, double octree_resolution = 0.1);
    // the same bytes in memory; the return value as above
    long long octomapBinary(std::vector<uint8_t> &out, double octree_resolution = 0.1);

    // a new map: globalMap is emptied (the mapper and its device scratch stay)
    void Reset();

    PointCloud globalMap;
    float mDepthMapFactor;   // 1: depth is in metres already

private:
    PointCloudMappingHIP(const PointCloudMappingHIP &);
    PointCloudMappingHIP &operator=(const PointCloudMappingHIP &);
    int run(float fx, float fy, float cx, float cy, const double *Twc16, const cv::Mat &color, const cv::Mat &depth, PointCloud *raw,
            PointCloud *filtered);
    double resolution;
    orbx_cloudmapper_t *mpMapper;
};

#endif
