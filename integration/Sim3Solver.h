// Sim3Solver.h -- replacement for orb_slam2/include/Sim3Solver.h in a
// reference tree that links liborbx.so.  The public interface is the
// reference's (Sim3Solver.h:40-50); the state behind it is OrbxSim3Solver's
// (include/orbx_orbslam2.hpp): the correspondences as the constructor collects
// them, the index triples of every RANSAC iteration, and the hypotheses the
// device computed from them.  iterate() walks those.
//
// OrbxPrepareSim3Solvers is the one addition: LoopClosing::ComputeSim3 calls
// it once after its constructor loop, and every solver's hypotheses are then
// one kernel launch.  A solver that was not prepared launches its own on the
// first iterate().
#ifndef SIM3SOLVER_H
#define SIM3SOLVER_H

#include <vector>

#include <opencv2/core/core.hpp>

#include "KeyFrame.h"
#include "orbx_orbslam2.hpp"

namespace ORB_SLAM2 {

class Sim3Solver {
public:
    Sim3Solver(KeyFrame *pKF1, KeyFrame *pKF2, const std::vector<MapPoint *> &vpMatched12,
               const bool bFixScale = true);

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300);

    cv::Mat find(std::vector<bool> &vbInliers12, int &nInliers);

    cv::Mat iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers);

    cv::Mat GetEstimatedRotation();
    cv::Mat GetEstimatedTranslation();
    float GetEstimatedScale();

protected:
    friend void OrbxPrepareSim3Solvers(std::vector<Sim3Solver *> &vpSolvers);
    OrbxSim3Solver mSolver;
};

// Draws every listed solver's triples (in list order, null entries skipped)
// and computes all their hypotheses in one launch.
void OrbxPrepareSim3Solvers(std::vector<Sim3Solver *> &vpSolvers);

}  // namespace ORB_SLAM2

#endif  // SIM3SOLVER_H
