// Recording stand-in for orbx_pose_optimization (the CPU half of
// tests/test_pose_forwarder.py): writes the arrays it was handed to the file
// $ORBX_POSE_RECORD and answers with a recognisable result, so the test sees
// both what the forwarder passed and what it did with the answer.
//
// Record: int32 device, n; float Tcw[12]; float cam[5]; n orbx_pose_obs;
//         int32 chi2_is_null, iterations_is_null.
// Answer: Tcw_out = Tcw with 1 added to its last element, outlier[k] = k % 2,
//         *n_inliers = n < 3 ? 0 : 1000 + n.
#include <cstdio>
#include <cstdlib>

#include "orbx.h"

extern "C" {

const char *orbx_strerror(int code) { return code == 0 ? "ok" : "error"; }

int orbx_pose_optimization(int device, const float *Tcw, const orbx_pose_camera *cam, const orbx_pose_obs *obs, int n,
                           float *Tcw_out, uint8_t *outlier, double *chi2, int *n_inliers, int *iterations) {
    const char *path = std::getenv("ORBX_POSE_RECORD");
    FILE *f = path ? std::fopen(path, "wb") : nullptr;
    if (!f || !Tcw || !cam || !Tcw_out || !n_inliers || n < 0 || (n && (!obs || !outlier))) return ORBX_EINVAL;
    const int32_t head[2] = {device, n}, tail[2] = {chi2 == nullptr, iterations == nullptr};
    std::fwrite(head, 4, 2, f);
    std::fwrite(Tcw, 4, 12, f);
    std::fwrite(cam, sizeof(*cam), 1, f);
    if (n) std::fwrite(obs, sizeof(*obs), n, f);
    std::fwrite(tail, 4, 2, f);
    std::fclose(f);
    for (int k = 0; k < 12; ++k) Tcw_out[k] = Tcw[k];
    Tcw_out[11] += 1.0f;
    for (int k = 0; k < n; ++k) outlier[k] = k % 2;
    *n_inliers = n < 3 ? 0 : 1000 + n;
    return ORBX_OK;
}

}  // extern "C"
