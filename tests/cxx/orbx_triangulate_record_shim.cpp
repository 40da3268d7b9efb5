// Recording stand-in for orbx_triangulate_batch (the CPU half of
// tests/test_triangulate_forwarder.py): appends what it was handed to the file
// $ORBX_TRI_RECORD and answers with a recognisable result, so the test sees
// both what the forwarder passed and what it did with the answer.
//
// Record, per call: int32 device, nproblems; nproblems orbx_tri_view v1, then
//         v2; nproblems float ratio_factor; nproblems + 1 int32 offsets; the
//         orbx_tri_pair of all problems.
// Answer: pair i of the call's problem p: X = (p, i, 0.5), status = (p + i) % 9.
#include <cstdio>
#include <cstdlib>

#include "orbx.h"

extern "C" {

const char *orbx_strerror(int code) { return code == 0 ? "ok" : "error"; }

int orbx_triangulate_batch(int device, const orbx_tri_view *v1, const orbx_tri_view *v2, const float *ratio_factor,
                           const orbx_tri_pair *pairs, const int32_t *offsets, int nproblems, orbx_tri_point *out) {
    const char *path = std::getenv("ORBX_TRI_RECORD");
    FILE *f = path ? std::fopen(path, "ab") : nullptr;
    if (!f || nproblems < 0 || !v1 || !v2 || !ratio_factor || !offsets) return ORBX_EINVAL;
    const int32_t head[2] = {device, nproblems};
    std::fwrite(head, 4, 2, f);
    std::fwrite(v1, sizeof(*v1), nproblems, f);
    std::fwrite(v2, sizeof(*v2), nproblems, f);
    std::fwrite(ratio_factor, 4, nproblems, f);
    std::fwrite(offsets, 4, nproblems + 1, f);
    if (offsets[nproblems]) std::fwrite(pairs, sizeof(*pairs), offsets[nproblems], f);
    std::fclose(f);
    for (int p = 0; p < nproblems; ++p)
        for (int i = 0; i < offsets[p + 1] - offsets[p]; ++i) {
            orbx_tri_point &o = out[offsets[p] + i];
            o.X[0] = (float)p;
            o.X[1] = (float)i;
            o.X[2] = 0.5f;
            o.status = (p + i) % 9;
        }
    return ORBX_OK;
}

}  // extern "C"
