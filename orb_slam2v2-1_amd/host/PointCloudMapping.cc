// PointCloudMapping.cc — see PointCloudMapping.h.  Host glue only: every point is computed by orbx_keyframe_cloud.
#include "PointCloudMapping.h"
#include <cstdio>
#include <cstdlib>

PointCloudMappingHIP::PointCloudMappingHIP(double resolution_) : mDepthMapFactor(1.0f), resolution(0.1), mpMapper(nullptr) {
    resolution = (resolution_ > 0) ? resolution_ : resolution;   // src/pointcloudmapping.cc:31
    const char *dev = std::getenv("ORBX_DEVICE");
    // step 3 (:87-89); alpha 255 (PCL >= 1.1's PointXYZRGBA constructor)
    if (orbx_cloudmapper_create((float)resolution, 3, 255, dev ? std::atoi(dev) : 0, &mpMapper) != ORBX_OK) {
        std::fprintf(stderr, "PointCloudMappingHIP: %s\n", orbx_last_error());
        mpMapper = nullptr;
    }
}

PointCloudMappingHIP::~PointCloudMappingHIP() { orbx_cloudmapper_destroy(mpMapper); }

int PointCloudMappingHIP::run(float fx, float fy, float cx, float cy, const double *Twc16, const cv::Mat &color, const cv::Mat &depth,
                              PointCloud *raw, PointCloud *filtered) {
    if (raw) raw->clear();
    filtered->clear();
    if (!mpMapper || !Twc16) return -1;
    if (color.empty() || depth.empty()) return 0;
    const int ch = color.channels();
    if (color.depth() != CV_8U || (ch != 3 && ch != 4) || depth.cols != color.cols || depth.rows != color.rows ||
        (depth.type() != CV_16U && depth.type() != CV_32F)) {
        std::fprintf(stderr, "PointCloudMappingHIP: CV_8UC3 / CV_8UC4 colour and CV_16U / CV_32F depth of one size expected\n");
        return -1;
    }
    const int cap = orbx_cloud_capacity(color.cols, color.rows, 3);
    if (raw) raw->resize(cap);
    filtered->resize(cap);
    int nr = 0, n = 0;
    const int rc = orbx_keyframe_cloud(mpMapper, color.ptr(0), ch, (int)color.step, depth.ptr(0), depth.type(), (int)depth.step,
                                       mDepthMapFactor, color.cols, color.rows, fx, fy, cx, cy, Twc16, cap, raw ? raw->data() : nullptr,
                                       &nr, filtered->data(), &n);
    if (rc != ORBX_OK) {
        std::fprintf(stderr, "PointCloudMappingHIP: %s\n", orbx_last_error());
        if (raw) raw->clear();
        filtered->clear();
        return -1;
    }
    if (raw) raw->resize(nr);
    filtered->resize(n);
    return n;
}

PointCloudMappingHIP::PointCloud PointCloudMappingHIP::generatePointCloud(float fx, float fy, float cx, float cy, const double *Twc16,
                                                                          const cv::Mat &color, const cv::Mat &depth) {
    PointCloud raw, filtered;
    run(fx, fy, cx, cy, Twc16, color, depth, &raw, &filtered);
    return raw;
}

int PointCloudMappingHIP::insertKeyFrame(float fx, float fy, float cx, float cy, const double *Twc16, const cv::Mat &color,
                                         const cv::Mat &depth) {
    PointCloud tmp;
    const int n = run(fx, fy, cx, cy, Twc16, color, depth, nullptr, &tmp);
    if (n < 0) return n;
    globalMap.insert(globalMap.end(), tmp.begin(), tmp.end());   // *globalMap += *tmp (:126)
    return n;
}

void PointCloudMappingHIP::Reset() { globalMap.clear(); }
