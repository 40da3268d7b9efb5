// Test stand-in for orb_slam2/include/Optimizer.h with the function
// integration/Optimizer_sim3_orbx.cc replaces (Optimizer.h:57), and for what
// that header brings in of g2o (types_seven_dof_expmap.h -> sim3.h): g2o::Sim3
// with its public accessors and the two Eigen types they speak, no more.
#pragma once
#include <vector>

#include "KeyFrame.h"
#include "MapPoint.h"

namespace Eigen {
struct Vector3d {
    double v[3];
    Vector3d() : v{0, 0, 0} {}
    Vector3d(double x, double y, double z) : v{x, y, z} {}
    double operator[](int i) const { return v[i]; }
    double &operator[](int i) { return v[i]; }
};
struct Vector4d {
    double v[4];
    double operator[](int i) const { return v[i]; }
    double &operator[](int i) { return v[i]; }
};
class Quaterniond {   // coefficients stored x, y, z, w; the constructor takes w first
public:
    Quaterniond() : c_{{0, 0, 0, 1}} {}
    Quaterniond(double w, double x, double y, double z) : c_{{x, y, z, w}} {}
    const Vector4d &coeffs() const { return c_; }
    Vector4d &coeffs() { return c_; }

private:
    Vector4d c_;
};
}  // namespace Eigen

namespace g2o {
struct Sim3 {
    Sim3() : s(1.) {}
    Sim3(const Eigen::Quaterniond &r_, const Eigen::Vector3d &t_, double s_) : r(r_), t(t_), s(s_) {}
    const Eigen::Vector3d &translation() const { return t; }
    const Eigen::Quaterniond &rotation() const { return r; }
    const double &scale() const { return s; }

protected:
    Eigen::Quaterniond r;
    Eigen::Vector3d t;
    double s;
};
}  // namespace g2o

namespace ORB_SLAM2 {
class Optimizer {
public:
    static int OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches1, g2o::Sim3 &g2oS12,
                            const float th2, const bool bFixScale);
};
}  // namespace ORB_SLAM2
