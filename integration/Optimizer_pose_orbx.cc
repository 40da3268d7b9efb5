// Optimizer_pose_orbx.cc -- Optimizer::PoseOptimization (orb_slam2/src/
// Optimizer.cc:265-509) for a reference tree that links liborbx.so.  The
// frame's observations are collected as :314-403 does (every feature with a
// map point, in feature order, its mvbOutlier cleared), the four rounds of
// Levenberg-Marquardt and the classification between them run on the device
// in one orbx_pose_optimization call, and the result is applied as :499-508.
// Replace only this function's body in Optimizer.cc.
//
// tests/cxx/pose_forwarder_test.cpp compiles this file against test stand-ins
// of the reference headers (tests/cxx/pose_mock/Optimizer.h declares the
// function) and checks it on the GPU against tests/pyref_pose.py, and on the
// CPU against a stand-in that records what it was handed.
#include <cstring>
#include <mutex>
#include <vector>

#include "Optimizer.h"
#include "orbx_orbslam2.hpp"

namespace ORB_SLAM2 {

namespace {
// unique_lock<mutex> lock(MapPoint::mGlobalMutex) (:311) where MapPoint has
// that member, as the reference's does
template <class MP>
auto lock_map_points(int) -> std::unique_lock<decltype(MP::mGlobalMutex)> {
    return std::unique_lock<decltype(MP::mGlobalMutex)>(MP::mGlobalMutex);
}
template <class MP>
int lock_map_points(long) {
    return 0;
}
}  // namespace

int Optimizer::PoseOptimization(Frame *pFrame) {
    const int N = pFrame->N;
    std::vector<orbx_pose_obs> obs;
    std::vector<size_t> vnIndexEdge;
    obs.reserve(N);
    vnIndexEdge.reserve(N);
    {
        auto lock = lock_map_points<MapPoint>(0);
        (void)lock;
        for (int i = 0; i < N; i++) {
            MapPoint *pMP = pFrame->mvpMapPoints[i];
            if (!pMP) continue;
            pFrame->mvbOutlier[i] = false;
            const cv::KeyPoint &kpUn = pFrame->mvKeysUn[i];
            const cv::Mat Xw = pMP->GetWorldPos();
            orbx_pose_obs o;
            for (int k = 0; k < 3; ++k) o.Xw[k] = Xw.at<float>(k);
            o.u = kpUn.pt.x;
            o.v = kpUn.pt.y;
            o.ur = pFrame->mvuRight[i];   // < 0: the monocular edge
            o.inv_sigma2 = pFrame->mvInvLevelSigma2[kpUn.octave];
            obs.push_back(o);
            vnIndexEdge.push_back(i);
        }
    }
    const int n = (int)obs.size();   // nInitialCorrespondences

    float Tcw[12], Tout[12];
    for (int r = 0; r < 3; ++r) std::memcpy(&Tcw[4 * r], pFrame->mTcw.ptr<float>(r), 4 * sizeof(float));
    const orbx_pose_camera cam = {pFrame->fx, pFrame->fy, pFrame->cx, pFrame->cy, pFrame->mbf};
    std::vector<uint8_t> outlier(n > 0 ? n : 1, 0);
    int nInliers = 0;
    orbx_detail::check(orbx_pose_optimization(orbx_detail::device_index(), Tcw, &cam, obs.data(), n, Tout,
                                              outlier.data(), nullptr, &nInliers, nullptr),
                       "PoseOptimization");
    if (n < 3) return 0;   // :408-409, before SetPose

    for (int k = 0; k < n; ++k) pFrame->mvbOutlier[vnIndexEdge[k]] = outlier[k] != 0;
    cv::Mat pose = cv::Mat::eye(4, 4, CV_32F);
    for (int r = 0; r < 3; ++r) std::memcpy(pose.ptr<float>(r), &Tout[4 * r], 4 * sizeof(float));
    pFrame->SetPose(pose);
    return nInliers;
}

}  // namespace ORB_SLAM2
