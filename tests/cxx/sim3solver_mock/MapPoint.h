// Test stand-in for orb_slam2/include/MapPoint.h with the members Sim3Solver's
// constructor reads.
#pragma once
#include <map>

#include <opencv2/core/core.hpp>

namespace ORB_SLAM2 {

class KeyFrame;

class MapPoint {
public:
    cv::Mat mWorldPos;   // 3x1 CV_32F
    bool mbBad = false;
    std::map<KeyFrame *, size_t> mObservations;

    cv::Mat GetWorldPos() const { return mWorldPos.clone(); }
    bool isBad() const { return mbBad; }
    int GetIndexInKeyFrame(KeyFrame *pKF) const {
        auto it = mObservations.find(pKF);
        return it == mObservations.end() ? -1 : (int)it->second;
    }
};

}  // namespace ORB_SLAM2
