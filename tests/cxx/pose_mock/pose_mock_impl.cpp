// The one out-of-line member of the stand-in Frame that the pose forwarder's
// test needs (Frame.cc:268-282), so that the test links without the rest of
// tests/cxx/orbslam_mock/mock_impl.cpp and the forwarders it refers to.
#include "Frame.h"

namespace ORB_SLAM2 {

void Frame::SetPose(const cv::Mat &Tcw) {
    mTcw = Tcw.clone();
    mRcw = mTcw.rowRange(0, 3).colRange(0, 3).clone();
    mtcw = mTcw.rowRange(0, 3).col(3).clone();
    mOw = -mRcw.t() * mtcw;
}

}  // namespace ORB_SLAM2
