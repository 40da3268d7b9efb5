// Recording stand-in for orbx_optimize_sim3 (the CPU half of
// tests/test_sim3_forwarder.py): writes what it was handed to the file
// $ORBX_SIM3_RECORD and answers with a recognisable result, so the test sees
// both what the forwarder passed and what it did with the answer.
//
// Record: int32 device, n; float th2; int32 fix_scale; orbx_sim3 S12;
//         orbx_sim3_camera cam1, cam2; n orbx_sim3_corr;
//         int32 chi2_12_is_null, chi2_21_is_null, iterations_is_null.
// Answer: S12_out = S12 with 1 added to t[2] and s doubled, *n_inliers =
//         1000 + n, removed[k] = k % 3; with $ORBX_SIM3_EARLY set removed[k] =
//         1 for every k >= 9 (nine survivors: the early return) and 0 below.
#include <cstdio>
#include <cstdlib>

#include "orbx.h"

extern "C" {

const char *orbx_strerror(int code) { return code == 0 ? "ok" : "error"; }

int orbx_optimize_sim3(int device, const orbx_sim3 *S12, const orbx_sim3_camera *cam1, const orbx_sim3_camera *cam2,
                       const orbx_sim3_corr *corr, int n, float th2, int fix_scale, orbx_sim3 *S12_out,
                       uint8_t *removed, double *chi2_12, double *chi2_21, int *n_inliers, int *iterations) {
    const char *path = std::getenv("ORBX_SIM3_RECORD");
    FILE *f = path ? std::fopen(path, "wb") : nullptr;
    if (!f || !S12 || !cam1 || !cam2 || !S12_out || !n_inliers || n < 0 || (n && (!corr || !removed)))
        return ORBX_EINVAL;
    const int32_t head[2] = {device, n}, fix = fix_scale;
    const int32_t tail[3] = {chi2_12 == nullptr, chi2_21 == nullptr, iterations == nullptr};
    std::fwrite(head, 4, 2, f);
    std::fwrite(&th2, 4, 1, f);
    std::fwrite(&fix, 4, 1, f);
    std::fwrite(S12, sizeof(*S12), 1, f);
    std::fwrite(cam1, sizeof(*cam1), 1, f);
    std::fwrite(cam2, sizeof(*cam2), 1, f);
    if (n) std::fwrite(corr, sizeof(*corr), n, f);
    std::fwrite(tail, 4, 3, f);
    std::fclose(f);
    *S12_out = *S12;
    S12_out->t[2] += 1.0;
    S12_out->s *= 2.0;
    const bool early = std::getenv("ORBX_SIM3_EARLY") != nullptr;
    for (int k = 0; k < n; ++k) removed[k] = early ? (k >= 9) : k % 3;
    *n_inliers = 1000 + n;
    return ORBX_OK;
}

}  // extern "C"
