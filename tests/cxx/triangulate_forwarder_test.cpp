// Driver of integration/LocalMapping_triangulate_orbx.cc for
// tests/test_triangulate_forwarder.py: reads a current keyframe, its
// neighbours and their pair lists from a file, builds them as the stand-in
// KeyFrames, makes the one OrbxTriangulateBatch call and writes what came back.
//
// in : int32 nk, levels; nk + 1 keyframes (the current one first): int32 N;
//      float Tcw[12], Ow[3], fx, fy, cx, cy, invfx, invfy, mbf, mb,
//      mfScaleFactor; float mvScaleFactors[levels], mvLevelSigma2[levels]; N
//      features of float u, v (mvKeysUn), raw_u, raw_v (mvKeys), ur, depth and
//      int32 octave; then per neighbour int32 npairs and npairs of int32 idx1, idx2
// out: int32 nk; per neighbour int32 count and count orbx_tri_point
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "orbx_forwarders.h"

using namespace ORB_SLAM2;

namespace {

FILE *in = nullptr;

template <typename T>
T rd() {
    T v;
    if (std::fread(&v, sizeof(T), 1, in) != 1) {
        std::fprintf(stderr, "short input\n");
        std::exit(2);
    }
    return v;
}

std::unique_ptr<KeyFrame> read_keyframe(int levels) {
    std::unique_ptr<KeyFrame> k(new KeyFrame);
    k->N = rd<int32_t>();
    k->Tcw = cv::Mat::zeros(4, 4, CV_32F);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) k->Tcw.at<float>(r, c) = rd<float>();
    k->Tcw.at<float>(3, 3) = 1.0f;
    k->Ow = cv::Mat::zeros(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r) k->Ow.at<float>(r) = rd<float>();
    k->fx = rd<float>(); k->fy = rd<float>(); k->cx = rd<float>(); k->cy = rd<float>();
    k->invfx = rd<float>(); k->invfy = rd<float>(); k->mbf = rd<float>(); k->mb = rd<float>();
    k->mfScaleFactor = rd<float>();
    k->mnScaleLevels = levels;
    for (int l = 0; l < levels; ++l) k->mvScaleFactors.push_back(rd<float>());
    for (int l = 0; l < levels; ++l) k->mvLevelSigma2.push_back(rd<float>());
    for (int i = 0; i < k->N; ++i) {
        const float u = rd<float>(), v = rd<float>(), ru = rd<float>(), rv = rd<float>();
        k->mvuRight.push_back(rd<float>());
        k->mvDepth.push_back(rd<float>());
        const int octave = rd<int32_t>();
        k->mvKeysUn.push_back(cv::KeyPoint(cv::Point2f(u, v), 31.0f, -1, 0, octave));
        k->mvKeys.push_back(cv::KeyPoint(cv::Point2f(ru, rv), 31.0f, -1, 0, octave));
    }
    k->mvpMapPoints.assign(k->N, nullptr);
    return k;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3 || !(in = std::fopen(argv[1], "rb"))) return 2;
    const int nk = rd<int32_t>(), levels = rd<int32_t>();
    std::vector<std::unique_ptr<KeyFrame>> kfs;
    for (int k = 0; k <= nk; ++k) kfs.push_back(read_keyframe(levels));
    std::vector<KeyFrame *> neigh;
    std::vector<std::vector<std::pair<size_t, size_t>>> pairs(nk);
    for (int k = 0; k < nk; ++k) {
        neigh.push_back(kfs[k + 1].get());
        const int np = rd<int32_t>();
        for (int i = 0; i < np; ++i) {
            const int a = rd<int32_t>(), b = rd<int32_t>();
            pairs[k].push_back(std::make_pair((size_t)a, (size_t)b));
        }
    }
    std::fclose(in);
    const std::vector<std::vector<orbx_tri_point>> pts = OrbxTriangulateBatch(kfs[0].get(), neigh, pairs);
    FILE *out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    const int32_t n = (int32_t)pts.size();
    std::fwrite(&n, 4, 1, out);
    for (const auto &p : pts) {
        const int32_t c = (int32_t)p.size();
        std::fwrite(&c, 4, 1, out);
        if (c) std::fwrite(p.data(), sizeof(orbx_tri_point), c, out);
    }
    std::fclose(out);
    return 0;
}
