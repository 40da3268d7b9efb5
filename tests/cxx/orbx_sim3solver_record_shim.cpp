// Recording stand-in for orbx_sim3_ransac_batch (the CPU half of
// tests/test_sim3solver_forwarder.py): appends what it was handed to the file
// $ORBX_RANSAC_RECORD and answers with a recognisable result, so the test sees
// both what the forwarder passed and what it did with the answer.
//
// Record, per call: int32 device, nproblems; per problem: orbx_sim3_camera
//         cam1, cam2; int32 fix_scale, n, h; n orbx_ransac_corr; 3 h int32.
// Answer: hypothesis k of the call's problem p: R[j] = 100 p + k + j / 16,
//         t[j] = -(k + j / 4), s = 2 + k, n_inliers = n - 1 and a mask without
//         correspondence p at k == 7 + p, n at k == 11 + p, n - 2 (without
//         correspondences 0 and 1) at k == 12 + p, else 3 (the first three).
#include <cstdio>
#include <cstdlib>

#include "orbx.h"

extern "C" {

const char *orbx_strerror(int code) { return code == 0 ? "ok" : "error"; }

int orbx_sim3_ransac_batch(int device, const orbx_sim3_camera *cam1, const orbx_sim3_camera *cam2,
                           const int32_t *fix_scale, const orbx_ransac_corr *corr, const int32_t *corr_offsets,
                           const int32_t *triples, const int32_t *hyp_offsets, int nproblems, orbx_ransac_hyp *hyp,
                           uint64_t *mask) {
    const char *path = std::getenv("ORBX_RANSAC_RECORD");
    FILE *f = path ? std::fopen(path, "ab") : nullptr;
    if (!f || nproblems < 0 || !cam1 || !cam2 || !fix_scale || !corr_offsets || !hyp_offsets || !hyp || !mask)
        return ORBX_EINVAL;
    const int32_t head[2] = {device, nproblems};
    std::fwrite(head, 4, 2, f);
    size_t w0 = 0;
    for (int p = 0; p < nproblems; ++p) {
        const int32_t n = corr_offsets[p + 1] - corr_offsets[p], h = hyp_offsets[p + 1] - hyp_offsets[p];
        const int32_t meta[3] = {fix_scale[p], n, h};
        std::fwrite(cam1 + p, sizeof(*cam1), 1, f);
        std::fwrite(cam2 + p, sizeof(*cam2), 1, f);
        std::fwrite(meta, 4, 3, f);
        if (n) std::fwrite(corr + corr_offsets[p], sizeof(*corr), n, f);
        if (h) std::fwrite(triples + 3 * (size_t)hyp_offsets[p], 4, 3 * (size_t)h, f);
        const size_t words = ((size_t)n + 63) / 64;
        for (int k = 0; k < h; ++k) {
            orbx_ransac_hyp &o = hyp[hyp_offsets[p] + k];
            for (int j = 0; j < 9; ++j) o.R[j] = 100.f * p + k + j / 16.f;
            for (int j = 0; j < 3; ++j) o.t[j] = -(k + j / 4.f);
            o.s = 2.f + k;
            uint64_t *m = mask + w0 + k * words;
            for (size_t w = 0; w < words; ++w) m[w] = 0;
            auto set = [&](int i) { m[i >> 6] |= uint64_t(1) << (i & 63); };
            int count = 0;
            for (int i = 0; i < n; ++i) {
                bool in = i < 3;
                if (k == 7 + p) in = i != p;
                if (k == 11 + p) in = true;
                if (k == 12 + p) in = i >= 2;
                if (in) {
                    set(i);
                    ++count;
                }
            }
            o.n_inliers = count;
        }
        w0 += (size_t)h * words;
    }
    std::fclose(f);
    return ORBX_OK;
}

}  // extern "C"
