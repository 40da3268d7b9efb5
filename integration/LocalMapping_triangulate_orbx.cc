// LocalMapping_triangulate_orbx.cc -- the inner loop of
// LocalMapping::CreateNewMapPoints (orb_slam2/src/LocalMapping.cc:334-480) for
// every neighbour of the current keyframe as one device batch (declared in
// orbx_forwarders.h).  One problem per neighbour, its pairs in
// SearchForTriangulation's order, filled from the members the reference loop
// reads; what depends on the order of the loop (CheckNewKeyFrames, a feature
// that got its point from an earlier neighbour, new MapPoint) stays with the
// caller's walk over the results.
//
// tests/cxx/triangulate_forwarder_test.cpp runs it against a recording
// stand-in of orbx_triangulate_batch (no GPU) and against liborbx.
#include <stdexcept>
#include <string>

#include "orbx_forwarders.h"

namespace ORB_SLAM2 {

namespace {

// One keyframe as the loop reads it (:252-270, :317-329)
orbx_tri_view tri_view(KeyFrame *pKF) {
    orbx_tri_view v;
    const cv::Mat Tcw = pKF->GetPose(), Ow = pKF->GetCameraCenter();
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) v.Tcw[4 * r + c] = Tcw.at<float>(r, c);
    for (int r = 0; r < 3; ++r) v.Ow[r] = Ow.at<float>(r);
    v.fx = pKF->fx; v.fy = pKF->fy; v.cx = pKF->cx; v.cy = pKF->cy;
    v.invfx = pKF->invfx; v.invfy = pKF->invfy; v.mbf = pKF->mbf; v.mb = pKF->mb;
    v.pad = 0.0f;
    return v;
}

// One feature: mvKeysUn for the rays and the reprojection, mvKeys for
// UnprojectStereo, the octave's entries of the two scale tables
orbx_tri_obs tri_obs(KeyFrame *pKF, size_t idx) {
    const cv::KeyPoint &kp = pKF->mvKeysUn[idx], &raw = pKF->mvKeys[idx];
    orbx_tri_obs o;
    o.u = kp.pt.x; o.v = kp.pt.y;
    o.ur = pKF->mvuRight[idx]; o.depth = pKF->mvDepth[idx];
    o.raw_u = raw.pt.x; o.raw_v = raw.pt.y;
    o.sigma2 = pKF->mvLevelSigma2[kp.octave]; o.scale = pKF->mvScaleFactors[kp.octave];
    return o;
}

}  // namespace

std::vector<std::vector<orbx_tri_point>> OrbxTriangulateBatch(
    KeyFrame *pKF1, const std::vector<KeyFrame *> &vpNeighKFs,
    const std::vector<std::vector<std::pair<size_t, size_t>>> &vPairs) {
    const size_t nk = vpNeighKFs.size();
    if (vPairs.size() != nk) throw std::invalid_argument("OrbxTriangulateBatch: one pair list per neighbour");
    std::vector<std::vector<orbx_tri_point>> out(nk);
    if (nk == 0) return out;
    const std::vector<orbx_tri_view> v1(nk, tri_view(pKF1));
    const std::vector<float> ratio(nk, 1.5f * pKF1->mfScaleFactor);
    std::vector<orbx_tri_view> v2;
    std::vector<int32_t> off(1, 0);
    std::vector<orbx_tri_pair> pairs;
    for (size_t i = 0; i < nk; ++i) {
        v2.push_back(tri_view(vpNeighKFs[i]));
        for (const auto &m : vPairs[i]) {
            orbx_tri_pair p;
            p.o1 = tri_obs(pKF1, m.first);
            p.o2 = tri_obs(vpNeighKFs[i], m.second);
            pairs.push_back(p);
        }
        off.push_back((int32_t)pairs.size());
    }
    std::vector<orbx_tri_point> pts(pairs.size());
    const int rc = orbx_triangulate_batch(0, v1.data(), v2.data(), ratio.data(), pairs.data(), off.data(), (int)nk,
                                          pts.data());
    if (rc != ORBX_OK) throw std::runtime_error(std::string("orbx_triangulate_batch: ") + orbx_strerror(rc));
    for (size_t i = 0; i < nk; ++i) out[i].assign(pts.begin() + off[i], pts.begin() + off[i + 1]);
    return out;
}

}  // namespace ORB_SLAM2
