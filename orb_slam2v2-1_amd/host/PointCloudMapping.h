// PointCloudMapping.h — the data-parallel part of the reference's dense map (include/pointcloudmapping.h, src/pointcloudmapping.cc:
// 29-34, 83-127) on an MI355X through include/orbx.h: generatePointCloud of an RGB-D keyframe and the pcl::VoxelGrid filter
// saveOctomap puts it through.  Plane segmentation, the axis swap, octomap insertion and PCD output (:139-279) stay with the caller,
// and so does the pose: Twc16 is what the reference computes with its own Eigen,
//     Eigen::Isometry3d T = ORB_SLAM2::Converter::toSE3Quat(kf->GetPose());  Eigen::Matrix4d Twc = T.inverse().matrix();
// handed over row-major (Twc16[4 * i + j] = Twc(i, j)).
#ifndef POINTCLOUDMAPPING_HIP_H
#define POINTCLOUDMAPPING_HIP_H

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
