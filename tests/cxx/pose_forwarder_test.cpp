// pose_forwarder_test IN OUT: reads a frame written by tests/
// test_pose_forwarder.py, fills a stand-in Frame (features without a map point
// interleaved), calls Optimizer::PoseOptimization (integration/
// Optimizer_pose_orbx.cc) and writes back the return value, whether SetPose
// ran, the frame's pose and mvbOutlier.
//
// IN  (little endian): int32 N; float Tcw[12]; float cam[5] (fx fy cx cy bf);
//     float inv_sigma2[8]; then N records {int32 has_point; float Xw[3];
//     float u, v, ur; int32 octave; int32 outlier_before}.
// OUT: int32 ret; int32 set_pose; float Tcw[12]; int32 outlier[N].
#include <cstdint>
#include <cstdio>
#include <vector>

#include "Optimizer.h"

using namespace ORB_SLAM2;

struct Rec {
    int32_t has_point;
    float Xw[3];
    float u, v, ur;
    int32_t octave, outlier_before;
};

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t N = 0;
    float Tcw[12], cam[5], inv[8];
    if (std::fread(&N, 4, 1, f) != 1 || std::fread(Tcw, 4, 12, f) != 12 || std::fread(cam, 4, 5, f) != 5 ||
        std::fread(inv, 4, 8, f) != 8)
        return 2;
    std::vector<Rec> recs(N);
    if (N && std::fread(recs.data(), sizeof(Rec), N, f) != (size_t)N) return 2;
    std::fclose(f);

    Frame F;
    F.N = N;
    F.fx = cam[0]; F.fy = cam[1]; F.cx = cam[2]; F.cy = cam[3]; F.mbf = cam[4];
    F.mvInvLevelSigma2.assign(inv, inv + 8);
    F.mvKeysUn.resize(N);
    F.mvuRight.resize(N);
    F.mvpMapPoints.assign(N, nullptr);
    F.mvbOutlier.assign(N, false);
    std::vector<MapPoint> points(N);
    for (int i = 0; i < N; ++i) {
        const Rec &r = recs[i];
        F.mvKeysUn[i].pt.x = r.u;
        F.mvKeysUn[i].pt.y = r.v;
        F.mvKeysUn[i].octave = r.octave;
        F.mvuRight[i] = r.ur;
        F.mvbOutlier[i] = r.outlier_before != 0;
        if (r.has_point) {
            cv::Mat X(3, 1, CV_32F);
            for (int k = 0; k < 3; ++k) X.at<float>(k) = r.Xw[k];
            points[i].SetWorldPos(X);
            F.mvpMapPoints[i] = &points[i];
        }
    }
    F.mTcw = cv::Mat::eye(4, 4, CV_32F);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) F.mTcw.at<float>(r, c) = Tcw[4 * r + c];
    // (mRcw stays empty until SetPose runs)

    const int32_t ret = Optimizer::PoseOptimization(&F);

    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    const int32_t set_pose = !F.mRcw.empty();
    float To[12];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) To[4 * r + c] = F.mTcw.at<float>(r, c);
    std::vector<int32_t> out(N);
    for (int i = 0; i < N; ++i) out[i] = F.mvbOutlier[i];
    std::fwrite(&ret, 4, 1, f);
    std::fwrite(&set_pose, 4, 1, f);
    std::fwrite(To, 4, 12, f);
    if (N) std::fwrite(out.data(), 4, N, f);
    std::fclose(f);
    return 0;
}
