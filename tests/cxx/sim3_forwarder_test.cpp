// sim3_forwarder_test IN OUT: reads two keyframes and a match list written by
// tests/test_sim3_forwarder.py, fills the stand-in KeyFrames and MapPoints,
// calls Optimizer::OptimizeSim3 (integration/Optimizer_sim3_orbx.cc) and
// writes back the return value, g2oS12 and which matches are still set.
//
// IN  (little endian): int32 N, N2; float th2; int32 fix_scale; double S12[8]
//     (q xyzw, t, s); float K1[4], K2[4] (fx fy cx cy); float T1w[12], T2w[12];
//     float inv_sigma2[8]; then N records {int32 match (0: vpMatches1[i] null);
//     int32 mp1 (0 null, 1 good, 2 bad); int32 mp2_bad; int32 i2 (the matched
//     point's index in KF2, -1: not observed there); float X1w[3], X2w[3];
//     float u1, v1; int32 octave1; float u2, v2; int32 octave2}.
// OUT: int32 ret; double S12[8]; int32 match_set[N].
#include <cstdint>
#include <cstdio>
#include <vector>

#include "Optimizer.h"

using namespace ORB_SLAM2;

struct Rec {
    int32_t match, mp1, mp2_bad, i2;
    float X1w[3], X2w[3];
    float u1, v1;
    int32_t octave1;
    float u2, v2;
    int32_t octave2;
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
    int32_t N = 0, N2 = 0, fix = 0;
    float th2 = 0, K1[4], K2[4], T1[12], T2[12], inv[8];
    double S[8];
    if (std::fread(&N, 4, 1, f) != 1 || std::fread(&N2, 4, 1, f) != 1 || std::fread(&th2, 4, 1, f) != 1 ||
        std::fread(&fix, 4, 1, f) != 1 || std::fread(S, 8, 8, f) != 8 || std::fread(K1, 4, 4, f) != 4 ||
        std::fread(K2, 4, 4, f) != 4 || std::fread(T1, 4, 12, f) != 12 || std::fread(T2, 4, 12, f) != 12 ||
        std::fread(inv, 4, 8, f) != 8)
        return 2;
    std::vector<Rec> recs(N);
    if (N && std::fread(recs.data(), sizeof(Rec), N, f) != (size_t)N) return 2;
    std::fclose(f);

    KeyFrame kf1, kf2;
    kf1.mK = calib_of(K1);
    kf2.mK = calib_of(K2);
    kf1.Tcw = pose_of(T1);
    kf2.Tcw = pose_of(T2);
    kf1.mvInvLevelSigma2.assign(inv, inv + 8);
    kf2.mvInvLevelSigma2.assign(inv, inv + 8);
    kf1.mvKeysUn.resize(N);
    kf2.mvKeysUn.resize(N2);
    kf1.mvpMapPoints.assign(N, nullptr);
    std::vector<MapPoint> points1(N), points2(N);
    std::vector<MapPoint *> matches(N, nullptr);
    for (int i = 0; i < N; ++i) {
        const Rec &r = recs[i];
        kf1.mvKeysUn[i].pt.x = r.u1;
        kf1.mvKeysUn[i].pt.y = r.v1;
        kf1.mvKeysUn[i].octave = r.octave1;
        if (r.mp1) {
            points1[i].mWorldPos = point_of(r.X1w);
            points1[i].mbBad = r.mp1 == 2;
            kf1.mvpMapPoints[i] = &points1[i];
        }
        if (r.match) {
            points2[i].mWorldPos = point_of(r.X2w);
            points2[i].mbBad = r.mp2_bad != 0;
            matches[i] = &points2[i];
            if (r.i2 >= 0) {
                if (r.i2 >= N2) return 2;
                points2[i].mObservations[&kf2] = r.i2;
                kf2.mvKeysUn[r.i2].pt.x = r.u2;
                kf2.mvKeysUn[r.i2].pt.y = r.v2;
                kf2.mvKeysUn[r.i2].octave = r.octave2;
            }
        }
    }
    g2o::Sim3 g2oS12(Eigen::Quaterniond(S[3], S[0], S[1], S[2]), Eigen::Vector3d(S[4], S[5], S[6]), S[7]);

    const int32_t ret = Optimizer::OptimizeSim3(&kf1, &kf2, matches, g2oS12, th2, fix != 0);

    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    double So[8];
    for (int k = 0; k < 4; ++k) So[k] = g2oS12.rotation().coeffs()[k];
    for (int k = 0; k < 3; ++k) So[4 + k] = g2oS12.translation()[k];
    So[7] = g2oS12.scale();
    std::vector<int32_t> set(N);
    for (int i = 0; i < N; ++i) set[i] = matches[i] != nullptr;
    std::fwrite(&ret, 4, 1, f);
    std::fwrite(So, 8, 8, f);
    if (N) std::fwrite(set.data(), 4, N, f);
    std::fclose(f);
    return 0;
}
