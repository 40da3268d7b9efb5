// triangulate_host.cpp -- orbx_triangulate.h compiled for the host, one thread:
// the project's restatement of a CreateNewMapPoints pair on a
// CPU.  The pairs run one after another; the results equal the device's bit for
// bit (no library function but sqrt is called).  tools/triangulate_probe.py
// times it as the CPU figure; tests/test_triangulate_host_text.py holds it to
// tests/pyref_triangulate.py.  Built by
// tools/triangulate_host/triangulate_host_build.py with
//   hipcc -x hip --offload-host-only -O3 -ffp-contract=off -shared -fPIC
#include "orbx_triangulate.h"

using namespace orbx;

extern "C" {

// out[offsets[nproblems]], sweeps (optional) likewise; returns -22 for what
// orbx_triangulate_batch rejects
int triangulate_host_batch(const orbx_tri_view *v1, const orbx_tri_view *v2, const float *ratio_factor,
                           const orbx_tri_pair *pairs, const int32_t *offsets, int nproblems, orbx_tri_point *out,
                           int32_t *sweeps) {
    if (nproblems < 0) return -22;
    if (nproblems == 0) return 0;
    if (offsets[0] != 0) return -22;
    for (int p = 0; p < nproblems; ++p)
        if (offsets[p + 1] < offsets[p]) return -22;
    const int n = offsets[nproblems];
    for (int i = 0; i < n; ++i)
        if (tri_obs_invalid(pairs[i].o1) || tri_obs_invalid(pairs[i].o2)) return -22;
    for (int i = 0; i < n; ++i) {
        const int p = tri_problem_of(offsets, nproblems, i);
        int sw = 0;
        out[i].status = tri_pair(v1[p], v2[p], ratio_factor[p], pairs[i].o1, pairs[i].o2, out[i].X, &sw);
        if (sweeps) sweeps[i] = sw;
    }
    return 0;
}

// The _device entry's behaviour: nothing validated, status 9 for an invalid pair
int triangulate_host_batch_unchecked(const orbx_tri_view *v1, const orbx_tri_view *v2, const float *ratio_factor,
                                     const orbx_tri_pair *pairs, const int32_t *offsets, int nproblems, int total_pairs,
                                     orbx_tri_point *out) {
    for (int i = 0; i < total_pairs; ++i) {
        const int p = tri_problem_of(offsets, nproblems, i);
        out[i].status = tri_pair(v1[p], v2[p], ratio_factor[p], pairs[i].o1, pairs[i].o2, out[i].X);
    }
    return 0;
}

// vt.row(3) of one row-major 4x4 (a matrix no pair reaches, such as one of rank 2); returns the sweeps
int triangulate_host_svd(const float *A, float *row) { return tri_svd_last_row(A, row); }

}  // extern "C"
