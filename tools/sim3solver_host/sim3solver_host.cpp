// sim3solver_host.cpp -- orbx_horn.h compiled for the host, one thread: the
// project's restatement of a Sim3Solver hypothesis on a CPU.
// The hypotheses run one after another, each over all correspondences; the
// results equal the device's bit for bit where the library's atan2, sin and
// cos agree.  tools/sim3solver_probe.py times it as the CPU figure;
// tests/test_sim3solver_host_text.py holds it to tests/pyref_sim3solver.py.
// Built by tools/sim3solver_host/sim3solver_host_build.py with
//   hipcc -x hip --offload-host-only -O3 -ffp-contract=off -shared -fPIC
#include <cstring>
#include <vector>

#include "orbx_horn.h"

using namespace orbx;

extern "C" {

// hyp[h], mask[h][(n + 63) / 64]; returns -22 for what orbx_sim3_ransac rejects
int sim3solver_host_ransac(const orbx_sim3_camera *cam1, const orbx_sim3_camera *cam2, int fix_scale,
                           const orbx_ransac_corr *corr, int n, const int32_t *triples, int h, orbx_ransac_hyp *hyp,
                           uint64_t *mask) {
    if (n < 0 || h < 0 || (h > 0 && n < 3)) return -22;
    for (int k = 0; k < h; ++k)
        if (!horn_triple_ok(triples + 3 * k, n)) return -22;
    const int words = (n + 63) / 64;
    std::vector<float> own(4 * (size_t)n);   // mvP1im1, mvP2im2
    for (int i = 0; i < n; ++i) {
        horn_own_projection(corr[i].X1c, *cam1, own[4 * i], own[4 * i + 1]);
        horn_own_projection(corr[i].X2c, *cam2, own[4 * i + 2], own[4 * i + 3]);
    }
    for (int k = 0; k < h; ++k) {
        float P1[3][3], P2[3][3], jac[kJacobiFloats];
        for (int i = 0; i < 3; ++i) {
            const orbx_ransac_corr &c = corr[triples[3 * k + i]];
            for (int r = 0; r < 3; ++r) {
                P1[r][i] = c.X1c[r];
                P2[r][i] = c.X2c[r];
            }
        }
        HornResult r;
        horn_compute(P1, P2, fix_scale, jac, 1, r);
        std::memcpy(hyp[k].R, r.R, sizeof(r.R));
        std::memcpy(hyp[k].t, r.t, sizeof(r.t));
        hyp[k].s = r.s;
        uint64_t *row = mask + (size_t)k * words;
        for (int w = 0; w < words; ++w) row[w] = 0;
        int count = 0;
        for (int i = 0; i < n; ++i)
            if (horn_inlier((const float *)r.T12, (const float *)r.T21, corr[i], *cam1, *cam2, own[4 * i],
                            own[4 * i + 1], own[4 * i + 2], own[4 * i + 3])) {
                row[i >> 6] |= uint64_t(1) << (i & 63);
                ++count;
            }
        hyp[k].n_inliers = count;
    }
    return 0;
}

}  // extern "C"
