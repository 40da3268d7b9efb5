// Sim3Solver_orbx.cc -- Sim3Solver (orb_slam2/src/Sim3Solver.cc:37-423) for a
// reference tree that links liborbx.so; replaces Sim3Solver.cc, with
// integration/Sim3Solver.h in place of the reference's header.  The
// constructor collects the correspondences as :62-103 does, with every skip
// kept (no match, no map point in KF1, either point bad, either point not
// observed in its keyframe); the points go to their keyframes' camera
// coordinates by the reference's own cv::Mat expression (:95, :98), and the
// thresholds keep the reference's truncation (mvnMaxError1/2 hold size_t).
// The index triples come from DUtils::Random::RandomInt with the reference's
// swap-with-last removal, all mRansacMaxIts of a solver when its hypotheses
// are launched, not five at a time: this changes only the order in which the
// process-global rand() stream is consumed, a stream Tracking's PnPsolver and
// Initializer share without a lock from another thread already.
//
// tests/cxx/sim3solver_forwarder_test.cpp compiles this file against test
// stand-ins of the reference headers (tests/cxx/sim3solver_mock) and checks it
// on the GPU against tests/pyref_sim3solver.py, and on the CPU against a
// stand-in that records what it was handed.
#include <vector>

#include "Sim3Solver.h"

#include "KeyFrame.h"
#include "MapPoint.h"

#include "Thirdparty/DBoW2/DUtils/Random.h"

namespace ORB_SLAM2 {

Sim3Solver::Sim3Solver(KeyFrame *pKF1, KeyFrame *pKF2, const std::vector<MapPoint *> &vpMatched12,
                       const bool bFixScale) {
    mSolver.fix_scale = bFixScale;
    const std::vector<MapPoint *> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
    const int mN1 = vpMatched12.size();
    mSolver.mN1 = mN1;
    mSolver.corr.reserve(mN1);
    mSolver.indices1.reserve(mN1);

    const cv::Mat Rcw1 = pKF1->GetRotation();
    const cv::Mat tcw1 = pKF1->GetTranslation();
    const cv::Mat Rcw2 = pKF2->GetRotation();
    const cv::Mat tcw2 = pKF2->GetTranslation();

    for (int i1 = 0; i1 < mN1; i1++) {
        if (!vpMatched12[i1]) continue;
        MapPoint *pMP1 = vpKeyFrameMP1[i1];
        MapPoint *pMP2 = vpMatched12[i1];
        if (!pMP1) continue;
        if (pMP1->isBad() || pMP2->isBad()) continue;
        const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1);
        const int indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
        if (indexKF1 < 0 || indexKF2 < 0) continue;

        const float sigmaSquare1 = pKF1->mvLevelSigma2[pKF1->mvKeysUn[indexKF1].octave];
        const float sigmaSquare2 = pKF2->mvLevelSigma2[pKF2->mvKeysUn[indexKF2].octave];
        const cv::Mat X3D1c = Rcw1 * pMP1->GetWorldPos() + tcw1;
        const cv::Mat X3D2c = Rcw2 * pMP2->GetWorldPos() + tcw2;

        orbx_ransac_corr c;
        for (int k = 0; k < 3; ++k) {
            c.X1c[k] = X3D1c.at<float>(k);
            c.X2c[k] = X3D2c.at<float>(k);
        }
        c.max_err1 = (float)(size_t)(9.210 * sigmaSquare1);
        c.max_err2 = (float)(size_t)(9.210 * sigmaSquare2);
        mSolver.corr.push_back(c);
        mSolver.indices1.push_back(i1);
    }

    const cv::Mat &K1 = pKF1->mK;
    const cv::Mat &K2 = pKF2->mK;
    mSolver.cam1 = {K1.at<float>(0, 0), K1.at<float>(1, 1), K1.at<float>(0, 2), K1.at<float>(1, 2)};
    mSolver.cam2 = {K2.at<float>(0, 0), K2.at<float>(1, 1), K2.at<float>(0, 2), K2.at<float>(1, 2)};

    SetRansacParameters();
}

void Sim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations) {
    mSolver.SetRansacParameters(probability, minInliers, maxIterations);
}

void OrbxPrepareSim3Solvers(std::vector<Sim3Solver *> &vpSolvers) {
    std::vector<OrbxSim3Solver *> todo;
    for (Sim3Solver *p : vpSolvers) {
        if (!p || p->mSolver.Launched()) continue;
        if (!p->mSolver.Drawn()) p->mSolver.Draw(DUtils::Random::RandomInt);
        todo.push_back(&p->mSolver);
    }
    OrbxSim3Solver::Prepare(todo);
}

cv::Mat Sim3Solver::iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers) {
    if (!mSolver.Launched()) {
        std::vector<Sim3Solver *> self(1, this);
        OrbxPrepareSim3Solvers(self);
    }
    const int k = mSolver.Iterate(nIterations, bNoMore, vbInliers, nInliers);
    if (k < 0) return cv::Mat();
    // mBestT12 = [ms12i * mR12i | mt12i] (:323-326)
    const orbx_ransac_hyp &h = mSolver.Hypothesis(k);
    cv::Mat T12 = cv::Mat::eye(4, 4, CV_32F);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T12.at<float>(r, c) = h.s * h.R[3 * r + c];
        T12.at<float>(r, 3) = h.t[r];
    }
    return T12;
}

cv::Mat Sim3Solver::find(std::vector<bool> &vbInliers12, int &nInliers) {
    bool bFlag;
    return iterate(mSolver.MaxIterations(), bFlag, vbInliers12, nInliers);
}

cv::Mat Sim3Solver::GetEstimatedRotation() {
    const orbx_ransac_hyp *b = mSolver.Best();
    if (!b) return cv::Mat();
    cv::Mat R(3, 3, CV_32F);
    for (int k = 0; k < 9; ++k) R.at<float>(k / 3, k % 3) = b->R[k];
    return R;
}

cv::Mat Sim3Solver::GetEstimatedTranslation() {
    const orbx_ransac_hyp *b = mSolver.Best();
    if (!b) return cv::Mat();
    cv::Mat t(3, 1, CV_32F);
    for (int k = 0; k < 3; ++k) t.at<float>(k) = b->t[k];
    return t;
}

float Sim3Solver::GetEstimatedScale() {
    const orbx_ransac_hyp *b = mSolver.Best();
    return b ? b->s : 0.f;
}

}  // namespace ORB_SLAM2
