// sim3solver_forwarder_test IN OUT: reads keyframe pairs and match lists
// written by tests/test_sim3solver_forwarder.py, fills the stand-in KeyFrames
// and MapPoints, and runs LoopClosing::ComputeSim3's solver loop
// (LoopClosing.cc:284-412 without its matcher and optimiser) over
// integration/Sim3Solver_orbx.cc: a Sim3Solver per candidate with
// SetRansacParameters(0.99, 20, 300), one OrbxPrepareSim3Solvers over the list
// (a null entry included, as discarded candidates leave), then iterate(5)
// round robin until every solver says bNoMore; the last solver's first call
// is find().
//
// IN  (little endian): int32 S, prepare; float sigma2[8]; per solver: int32 N,
//     N1, N2, fix; float K1[4], K2[4] (fx fy cx cy), T1w[12], T2w[12]; N
//     records {int32 match (0: vpMatched12[i] null); int32 mp1 (0 null, 1 good,
//     2 bad); int32 mp2_bad; int32 i1, i2 (the points' indices in KF1 / KF2,
//     -1: not observed there); float X1w[3], X2w[3]; int32 octave1, octave2}.
// OUT: int32 RandomInt calls after the preparation; then per iterate() call
//     {int32 solver, returned, bNoMore, nInliers; uint8 vbInliers[N]; if
//     returned: float T12[16], R[9], t[3], s}; then int32 -1 and the final
//     number of RandomInt calls.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "MapPoint.h"
#include "Sim3Solver.h"
#include "Thirdparty/DBoW2/DUtils/Random.h"

using namespace ORB_SLAM2;

struct Rec {
    int32_t match, mp1, mp2_bad, i1, i2;
    float X1w[3], X2w[3];
    int32_t octave1, octave2;
};

struct Candidate {
    KeyFrame kf1, kf2;
    std::vector<MapPoint> points1, points2;
    std::vector<MapPoint *> matches;
    int32_t fix = 0;
};

static cv::Mat pose_of(const float *T) {
    cv::Mat m = cv::Mat::eye(4, 4, CV_32F);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) m.at<float>(r, c) = T[4 * r + c];
    return m;
}

static cv::Mat calib_of(const float *k) {
    cv::Mat m = cv::Mat::eye(3, 3, CV_32F);
    m.at<float>(0, 0) = k[0];
    m.at<float>(1, 1) = k[1];
    m.at<float>(0, 2) = k[2];
    m.at<float>(1, 2) = k[3];
    return m;
}

static cv::Mat point_of(const float *x) {
    cv::Mat X(3, 1, CV_32F);
    for (int k = 0; k < 3; ++k) X.at<float>(k) = x[k];
    return X;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t S = 0, prepare = 0;
    float sigma2[8];
    if (std::fread(&S, 4, 1, f) != 1 || std::fread(&prepare, 4, 1, f) != 1 || std::fread(sigma2, 4, 8, f) != 8) return 2;
    std::vector<std::unique_ptr<Candidate>> cands;
    for (int s = 0; s < S; ++s) {
        int32_t head[4];
        float K1[4], K2[4], T1[12], T2[12];
        if (std::fread(head, 4, 4, f) != 4 || std::fread(K1, 4, 4, f) != 4 || std::fread(K2, 4, 4, f) != 4 ||
            std::fread(T1, 4, 12, f) != 12 || std::fread(T2, 4, 12, f) != 12)
            return 2;
        const int32_t N = head[0], N1 = head[1], N2 = head[2];
        std::vector<Rec> recs(N);
        if (N && std::fread(recs.data(), sizeof(Rec), N, f) != (size_t)N) return 2;
        cands.emplace_back(new Candidate);
        Candidate &c = *cands.back();
        c.fix = head[3];
        c.kf1.mK = calib_of(K1);
        c.kf2.mK = calib_of(K2);
        c.kf1.Tcw = pose_of(T1);
        c.kf2.Tcw = pose_of(T2);
        c.kf1.mvLevelSigma2.assign(sigma2, sigma2 + 8);
        c.kf2.mvLevelSigma2.assign(sigma2, sigma2 + 8);
        c.kf1.mvKeysUn.resize(N1);
        c.kf2.mvKeysUn.resize(N2);
        c.kf1.mvpMapPoints.assign(N, nullptr);
        c.points1.resize(N);
        c.points2.resize(N);
        c.matches.assign(N, nullptr);
        for (int i = 0; i < N; ++i) {
            const Rec &r = recs[i];
            if (r.i1 >= N1 || r.i2 >= N2) return 2;
            if (r.mp1) {
                c.points1[i].mWorldPos = point_of(r.X1w);
                c.points1[i].mbBad = r.mp1 == 2;
                c.kf1.mvpMapPoints[i] = &c.points1[i];
                if (r.i1 >= 0) {
                    c.points1[i].mObservations[&c.kf1] = r.i1;
                    c.kf1.mvKeysUn[r.i1].octave = r.octave1;
                }
            }
            if (r.match) {
                c.points2[i].mWorldPos = point_of(r.X2w);
                c.points2[i].mbBad = r.mp2_bad != 0;
                c.matches[i] = &c.points2[i];
                if (r.i2 >= 0) {
                    c.points2[i].mObservations[&c.kf2] = r.i2;
                    c.kf2.mvKeysUn[r.i2].octave = r.octave2;
                }
            }
        }
    }
    std::fclose(f);

    std::vector<std::unique_ptr<Sim3Solver>> own;
    std::vector<Sim3Solver *> vpSim3Solvers;
    for (int s = 0; s < S; ++s) {
        Candidate &c = *cands[s];
        own.emplace_back(new Sim3Solver(&c.kf1, &c.kf2, c.matches, c.fix != 0));
        own.back()->SetRansacParameters(0.99, 20, 300);
        if (s == 1) vpSim3Solvers.push_back(nullptr);
        vpSim3Solvers.push_back(own.back().get());
    }
    if (prepare) OrbxPrepareSim3Solvers(vpSim3Solvers);

    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    int32_t calls = DUtils::Random::Calls();
    std::fwrite(&calls, 4, 1, f);
    std::vector<bool> alive(S, true);
    std::vector<bool> first(S, true);
    for (bool any = S > 0; any;) {
        any = false;
        for (int s = 0; s < S; ++s) {
            if (!alive[s]) continue;
            Sim3Solver *p = own[s].get();
            std::vector<bool> vbInliers;
            int nInliers = -1;
            bool bNoMore = false;
            cv::Mat T;
            if (s == S - 1 && first[s])
                T = p->find(vbInliers, nInliers);
            else
                T = p->iterate(5, bNoMore, vbInliers, nInliers);
            first[s] = false;
            const int32_t ev[4] = {s, !T.empty(), bNoMore, nInliers};
            std::fwrite(ev, 4, 4, f);
            for (size_t i = 0; i < vbInliers.size(); ++i) {
                const uint8_t b = vbInliers[i];
                std::fwrite(&b, 1, 1, f);
            }
            if (!T.empty()) {
                const cv::Mat R = p->GetEstimatedRotation(), t = p->GetEstimatedTranslation();
                const float sc = p->GetEstimatedScale();
                for (int r = 0; r < 4; ++r) std::fwrite(T.ptr<float>(r), 4, 4, f);
                for (int r = 0; r < 3; ++r) std::fwrite(R.ptr<float>(r), 4, 3, f);
                for (int r = 0; r < 3; ++r) std::fwrite(t.ptr<float>(r), 4, 1, f);
                std::fwrite(&sc, 4, 1, f);
            }
            if (bNoMore) alive[s] = false;
            any = any || alive[s];
        }
    }
    const int32_t end = -1;
    calls = DUtils::Random::Calls();
    std::fwrite(&end, 4, 1, f);
    std::fwrite(&calls, 4, 1, f);
    std::fclose(f);
    return 0;
}
