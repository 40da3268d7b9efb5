// Test stand-in for orb_slam2/include/Optimizer.h with the two functions
// integration/ replaces (Optimizer.h:45, :51).  It goes before
// tests/cxx/orbslam_mock on the include path of the pose forwarder's test.
#pragma once
#include "Frame.h"

namespace ORB_SLAM2 {
class Optimizer {
public:
    void static LocalBundleAdjustment(KeyFrame *pKF, bool *pbStopFlag, Map *pMap);
    int static PoseOptimization(Frame *pFrame);
};
}  // namespace ORB_SLAM2
