// g2o_shim.h — g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3.h) and the three ORB_SLAM2::Converter functions around it
// (src/Converter.cc), reduced to what Optimizer::OptimizeSim3 and its caller touch (src/LoopClosing.cc:335-345): the
// (Matrix3d, Vector3d, double) constructor, operator*, inverse, map, rotation / translation / scale, Converter::toMatrix3d,
// toVector3d and toCvMat(g2o::Sim3).  For building the host classes where g2o and Eigen are absent (this image); define
// ORBX_HAVE_ORBSLAM2 and the reference's own "Converter.h" (which brings g2o's sim3.h and Eigen) is used instead.  The arithmetic is
// Eigen's, operation for operation: Quaterniond(Matrix3d) is Shoemake's conversion without normalisation, Quaterniond * Vector3d is
// _transformVector, toRotationMatrix the usual twelve products - the same statements as csrc/orbx_sim3opt.hip.
#pragma once
#ifdef ORBX_HAVE_ORBSLAM2
#include "Converter.h"
#include "LoopClosing.h"
#else
#include <cmath>
#include <functional>
#include <map>
#include "cv_shim.h"

namespace Eigen {
struct Vector3d {
    double v[3];
    Vector3d() { v[0] = v[1] = v[2] = 0.; }
    Vector3d(double x, double y, double z) { v[0] = x; v[1] = y; v[2] = z; }
    double &operator[](int i) { return v[i]; }
    const double &operator[](int i) const { return v[i]; }
    double &operator()(int i) { return v[i]; }
    const double &operator()(int i) const { return v[i]; }
};
struct Matrix3d {
    double m[3][3];
    Matrix3d() { for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) m[r][c] = 0.; }
    double &operator()(int r, int c) { return m[r][c]; }
    const double &operator()(int r, int c) const { return m[r][c]; }
};
class Quaterniond {
public:
    Quaterniond() : x_(0.), y_(0.), z_(0.), w_(1.) {}
    Quaterniond(double w, double x, double y, double z) : x_(x), y_(y), z_(z), w_(w) {}   // Eigen's order: w first
    explicit Quaterniond(const Matrix3d &R) {
        double t = R(0, 0) + R(1, 1) + R(2, 2);
        if (t > 0.) {
            t = std::sqrt(t + 1.0);
            w_ = 0.5 * t;
            t = 0.5 / t;
            x_ = (R(2, 1) - R(1, 2)) * t; y_ = (R(0, 2) - R(2, 0)) * t; z_ = (R(1, 0) - R(0, 1)) * t;
        } else {
            int i = 0;
            if (R(1, 1) > R(0, 0)) i = 1;
            if (R(2, 2) > R(i, i)) i = 2;
            const int j = (i + 1) % 3, k = (j + 1) % 3;
            t = std::sqrt(R(i, i) - R(j, j) - R(k, k) + 1.0);
            double v[3];
            v[i] = 0.5 * t;
            t = 0.5 / t;
            w_ = (R(k, j) - R(j, k)) * t;
            v[j] = (R(j, i) + R(i, j)) * t;
            v[k] = (R(k, i) + R(i, k)) * t;
            x_ = v[0]; y_ = v[1]; z_ = v[2];
        }
    }
    double x() const { return x_; }
    double y() const { return y_; }
    double z() const { return z_; }
    double w() const { return w_; }
    double &x() { return x_; }
    double &y() { return y_; }
    double &z() { return z_; }
    double &w() { return w_; }
    void setIdentity() { x_ = y_ = z_ = 0.; w_ = 1.; }
    Quaterniond conjugate() const { return Quaterniond(w_, -x_, -y_, -z_); }
    Quaterniond operator*(const Quaterniond &b) const {
        return Quaterniond(((w_ * b.w_ - x_ * b.x_) - y_ * b.y_) - z_ * b.z_, ((w_ * b.x_ + x_ * b.w_) + y_ * b.z_) - z_ * b.y_,
                           ((w_ * b.y_ + y_ * b.w_) + z_ * b.x_) - x_ * b.z_, ((w_ * b.z_ + z_ * b.w_) + x_ * b.y_) - y_ * b.x_);
    }
    Vector3d operator*(const Vector3d &v) const {   // _transformVector
        double uv[3] = {y_ * v[2] - z_ * v[1], z_ * v[0] - x_ * v[2], x_ * v[1] - y_ * v[0]};
        uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
        return Vector3d((v[0] + w_ * uv[0]) + (y_ * uv[2] - z_ * uv[1]), (v[1] + w_ * uv[1]) + (z_ * uv[0] - x_ * uv[2]),
                        (v[2] + w_ * uv[2]) + (x_ * uv[1] - y_ * uv[0]));
    }
    Matrix3d toRotationMatrix() const {
        const double tx = 2.0 * x_, ty = 2.0 * y_, tz = 2.0 * z_;
        const double twx = tx * w_, twy = ty * w_, twz = tz * w_, txx = tx * x_, txy = ty * x_, txz = tz * x_;
        const double tyy = ty * y_, tyz = tz * y_, tzz = tz * z_;
        Matrix3d R;
        R(0, 0) = 1.0 - (tyy + tzz); R(0, 1) = txy - twz; R(0, 2) = txz + twy;
        R(1, 0) = txy + twz; R(1, 1) = 1.0 - (txx + tzz); R(1, 2) = tyz - twx;
        R(2, 0) = txz - twy; R(2, 1) = tyz + twx; R(2, 2) = 1.0 - (txx + tyy);
        return R;
    }
private:
    double x_, y_, z_, w_;
};
}  // namespace Eigen

namespace g2o {
struct Sim3 {   // sim3.h:41-292
    Sim3() : s(1.) {}
    Sim3(const Eigen::Quaterniond &r_, const Eigen::Vector3d &t_, double s_) : r(r_), t(t_), s(s_) {}
    Sim3(const Eigen::Matrix3d &R, const Eigen::Vector3d &t_, double s_) : r(Eigen::Quaterniond(R)), t(t_), s(s_) {}
    Eigen::Vector3d map(const Eigen::Vector3d &xyz) const {
        const Eigen::Vector3d p = r * xyz;
        return Eigen::Vector3d(s * p[0] + t[0], s * p[1] + t[1], s * p[2] + t[2]);
    }
    Sim3 inverse() const {
        const double k = -1. / s;
        return Sim3(r.conjugate(), r.conjugate() * Eigen::Vector3d(k * t[0], k * t[1], k * t[2]), 1. / s);
    }
    Sim3 operator*(const Sim3 &other) const {   // the quaternion product is not normalised
        Sim3 ret;
        ret.r = r * other.r;
        ret.t = map(other.t);
        ret.s = s * other.s;
        return ret;
    }
    const Eigen::Vector3d &translation() const { return t; }
    Eigen::Vector3d &translation() { return t; }
    const Eigen::Quaterniond &rotation() const { return r; }
    Eigen::Quaterniond &rotation() { return r; }
    const double &scale() const { return s; }
    double &scale() { return s; }
protected:
    Eigen::Quaterniond r;
    Eigen::Vector3d t;
    double s;
};
}  // namespace g2o

// ORB_SLAM2::LoopClosing with its KeyFrameAndPose (include/LoopClosing.h:50-51, without Eigen's allocator), the name
// Optimizer::OptimizeEssentialGraph's signature needs.  LoopClosing.h includes this header first: whichever of the two comes first,
// g2o::Sim3 is complete when the class is declared
#include "LoopClosing.h"

namespace ORB_SLAM2 {
class Converter {   // src/Converter.cc:105-151
public:
    static Eigen::Matrix3d toMatrix3d(const cv::Mat &cvMat3) {
        Eigen::Matrix3d M;
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) M(r, c) = cvMat3.at<float>(r, c);
        return M;
    }
    static Eigen::Vector3d toVector3d(const cv::Mat &cvVector) {
        return Eigen::Vector3d(cvVector.at<float>(0), cvVector.at<float>(1), cvVector.at<float>(2));
    }
    static cv::Mat toCvMat(const g2o::Sim3 &Sim3) {   // toCvMat(s * eigR, eigt): the 4x4 CV_32F
        const Eigen::Matrix3d eigR = Sim3.rotation().toRotationMatrix();
        const Eigen::Vector3d eigt = Sim3.translation();
        const double s = Sim3.scale();
        cv::Mat cvMat = cv::Mat::eye(4, 4, CV_32F);
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) cvMat.at<float>(i, j) = (float)(s * eigR(i, j));
            cvMat.at<float>(i, 3) = (float)eigt(i);
        }
        return cvMat;
    }
};
}  // namespace ORB_SLAM2
#endif
