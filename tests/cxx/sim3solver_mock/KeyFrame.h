// Test stand-in for orb_slam2/include/KeyFrame.h with the members Sim3Solver's
// constructor reads (integration/Sim3Solver_orbx.cc), over the cv mock.
// tests/cxx/sim3solver_mock goes before tests/cxx/orbslam_mock on the include
// path of the Sim3Solver forwarder's test.
#pragma once
#include <vector>

#include <opencv2/core/core.hpp>

namespace ORB_SLAM2 {

class MapPoint;

class KeyFrame {
public:
    cv::Mat mK;    // 3x3 CV_32F
    cv::Mat Tcw;   // 4x4 CV_32F
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvLevelSigma2;
    std::vector<MapPoint *> mvpMapPoints;

    cv::Mat GetRotation() const { return Tcw.rowRange(0, 3).colRange(0, 3).clone(); }
    cv::Mat GetTranslation() const { return Tcw.rowRange(0, 3).col(3).clone(); }
    std::vector<MapPoint *> GetMapPointMatches() const { return mvpMapPoints; }
};

}  // namespace ORB_SLAM2
