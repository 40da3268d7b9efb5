// Optimizer_sim3_orbx.cc -- Optimizer::OptimizeSim3 (orb_slam2/src/
// Optimizer.cc:1177-1414) for a reference tree that links liborbx.so.  The
// correspondences are collected as :1238-1335 does (a match, both map points
// present and good, the matched point observed in pKF2; vnIndexEdge kept), the
// points go to their keyframes' camera coordinates by the reference's own
// cv::Mat expression, the two rounds of Levenberg-Marquardt and the two
// classifications run on the device in one orbx_optimize_sim3 call, and the
// result is applied as :1345-1413.  Replace only this function's body in
// Optimizer.cc.
//
// tests/cxx/sim3_forwarder_test.cpp compiles this file against test stand-ins
// of the reference headers (tests/cxx/sim3_mock) and checks it on the GPU
// against tests/pyref_sim3.py, and on the CPU against a stand-in that records
// what it was handed.
#include <vector>

#include "Optimizer.h"
#include "orbx_orbslam2.hpp"

namespace ORB_SLAM2 {

int Optimizer::OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches1, g2o::Sim3 &g2oS12,
                            const float th2, const bool bFixScale) {
    const cv::Mat &K1 = pKF1->mK;
    const cv::Mat &K2 = pKF2->mK;
    const cv::Mat R1w = pKF1->GetRotation();
    const cv::Mat t1w = pKF1->GetTranslation();
    const cv::Mat R2w = pKF2->GetRotation();
    const cv::Mat t2w = pKF2->GetTranslation();
    const orbx_sim3_camera cam1 = {K1.at<float>(0, 0), K1.at<float>(1, 1), K1.at<float>(0, 2), K1.at<float>(1, 2)};
    const orbx_sim3_camera cam2 = {K2.at<float>(0, 0), K2.at<float>(1, 1), K2.at<float>(0, 2), K2.at<float>(1, 2)};

    const int N = vpMatches1.size();
    const std::vector<MapPoint *> vpMapPoints1 = pKF1->GetMapPointMatches();
    std::vector<orbx_sim3_corr> corr;
    std::vector<size_t> vnIndexEdge;
    corr.reserve(N);
    vnIndexEdge.reserve(N);
    for (int i = 0; i < N; i++) {
        if (!vpMatches1[i]) continue;
        MapPoint *pMP1 = vpMapPoints1[i];
        MapPoint *pMP2 = vpMatches1[i];
        const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
        if (!pMP1 || !pMP2) continue;
        if (pMP1->isBad() || pMP2->isBad() || i2 < 0) continue;
        const cv::Mat P3D1w = pMP1->GetWorldPos();
        const cv::Mat P3D1c = R1w * P3D1w + t1w;
        const cv::Mat P3D2w = pMP2->GetWorldPos();
        const cv::Mat P3D2c = R2w * P3D2w + t2w;
        const cv::KeyPoint &kpUn1 = pKF1->mvKeysUn[i];
        const cv::KeyPoint &kpUn2 = pKF2->mvKeysUn[i2];
        orbx_sim3_corr c;
        for (int k = 0; k < 3; ++k) {
            c.P1c[k] = P3D1c.at<float>(k);
            c.P2c[k] = P3D2c.at<float>(k);
        }
        c.u1 = kpUn1.pt.x;
        c.v1 = kpUn1.pt.y;
        c.inv_sigma2_1 = pKF1->mvInvLevelSigma2[kpUn1.octave];
        c.u2 = kpUn2.pt.x;
        c.v2 = kpUn2.pt.y;
        c.inv_sigma2_2 = pKF2->mvInvLevelSigma2[kpUn2.octave];
        corr.push_back(c);
        vnIndexEdge.push_back(i);
    }
    const int nCorrespondences = (int)corr.size();

    orbx_sim3 S12, S12_out;
    for (int k = 0; k < 4; ++k) S12.q[k] = g2oS12.rotation().coeffs()[k];
    for (int k = 0; k < 3; ++k) S12.t[k] = g2oS12.translation()[k];
    S12.s = g2oS12.scale();
    std::vector<uint8_t> removed(nCorrespondences > 0 ? nCorrespondences : 1, 0);
    int nIn = 0;
    orbx_detail::check(orbx_optimize_sim3(orbx_detail::device_index(), &S12, &cam1, &cam2, corr.data(),
                                          nCorrespondences, th2, bFixScale ? 1 : 0, &S12_out, removed.data(), nullptr,
                                          nullptr, &nIn, nullptr),
                       "OptimizeSim3");

    int nBad = 0;
    for (int k = 0; k < nCorrespondences; ++k) {
        if (removed[k]) vpMatches1[vnIndexEdge[k]] = static_cast<MapPoint *>(NULL);   // :1361, :1402
        if (removed[k] == 1) nBad++;
    }
    if (nCorrespondences - nBad < 10) return 0;   // :1379-1380, before g2oS12 is written

    g2oS12 = g2o::Sim3(Eigen::Quaterniond(S12_out.q[3], S12_out.q[0], S12_out.q[1], S12_out.q[2]),
                       Eigen::Vector3d(S12_out.t[0], S12_out.t[1], S12_out.t[2]), S12_out.s);
    return nIn;
}

}  // namespace ORB_SLAM2
