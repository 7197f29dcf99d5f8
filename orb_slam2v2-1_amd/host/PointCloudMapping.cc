// PointCloudMapping.cc — see PointCloudMapping.h.  Host glue only: every point is computed by orbx_keyframe_cloud, every byte of the
// tree by orbx_octomap_bt.
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

long long PointCloudMappingHIP::octomapBinary(std::vector<uint8_t> &out, double octree_resolution) {
    out.clear();
    if (!mpMapper || globalMap.size() > 0x7fffffffu) return -1;
    const int n = (int)globalMap.size();
    // room for one inner node per point (a surface has about a third as many); the exact size, which the call reports, otherwise
    out.resize(192 + 2 * (size_t)n);
    orbx_octree_info_t info;
    size_t bytes = 0;
    int rc = orbx_octomap_bt(mpMapper, globalMap.data(), n, nullptr, octree_resolution, out.data(), out.size(), &bytes, &info);
    if (rc == ORBX_ERR_CAPACITY) {
        out.resize(bytes);
        rc = orbx_octomap_bt(mpMapper, globalMap.data(), n, nullptr, octree_resolution, out.data(), out.size(), &bytes, &info);
    }
    if (rc != ORBX_OK) {
        std::fprintf(stderr, "PointCloudMappingHIP: %s\n", orbx_last_error());
        out.clear();
        return -1;
    }
    out.resize(bytes);
    return (long long)info.tree_size;
}

long long PointCloudMappingHIP::saveOctomap(const char *oct_name, double octree_resolution) {
    std::vector<uint8_t> bytes;
    const long long size = octomapBinary(bytes, octree_resolution);
    if (size < 0 || !oct_name) return -1;
    FILE *f = std::fopen(oct_name, "wb");
    if (!f) {
        std::fprintf(stderr, "PointCloudMappingHIP: cannot write %s\n", oct_name);
        return -1;
    }
    const bool ok = std::fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    return (std::fclose(f) == 0 && ok) ? size : -1;
}

void PointCloudMappingHIP::Reset() { globalMap.clear(); }
