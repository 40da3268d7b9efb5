// sim3_host.cpp -- orbx_sim3.h, and orbx_lm.h under it, compiled for the host,
// one thread: the project's restatement of Optimizer::OptimizeSim3 (DESIGN.md
// §3.14) on a CPU.  The
// executor runs the 64 lanes of the device's wave one after another and adds
// their partials in lane order, so the results equal the device's bit for bit
// (the update's sin / cos are the host's libm here).  tools/sim3_probe.py
// times it as the CPU figure; tests/test_sim3_host_text.py holds it to
// tests/pyref_sim3.py.  Built by tools/sim3_host/sim3_host_build.py with
//   hipcc -x hip --offload-host-only -O3 -ffp-contract=off -shared -fPIC
#include <cstring>
#include <vector>

#include "orbx_sim3.h"

using namespace orbx;

namespace {

struct HostExec {
    Sim3Problem pr;
    uint8_t *flags;   // the removal flags (pr.flag when the full run drives it)

    void build(const Sim3 &S, double *H, double *b, double *chi) {
        Sim3 tab[kSim3Table], tabinv[kSim3Table];
        for (int k = 0; k < kSim3Table; ++k) sim3_table_entry(S, k, pr.fix_scale, tab[k], tabinv[k]);
        const Sim3TableRef ref = {tab, tabinv};
        double tot[kSim3Sums];
        for (int l = 0; l < kSim3Lanes; ++l) {
            double acc[kSim3Sums];
            for (int f = 0; f < kSim3Sums; ++f) acc[f] = 0.0;
            sim3_lane_build(pr, ref, l, acc);
            for (int f = 0; f < kSim3Sums; ++f) tot[f] = l == 0 ? acc[f] : tot[f] + acc[f];
        }
        lm_unpack<7>(tot, H, b, chi);
    }

    double errors(const Sim3 &S) {
        Sim3 Sinv;
        sim3_inverse(S, Sinv);
        double tot = 0;
        for (int l = 0; l < kSim3Lanes; ++l) {
            const double a = sim3_lane_errors(pr, S, Sinv, l);
            tot = l == 0 ? a : tot + a;
        }
        return tot;
    }

    void update(Sim3 &S, const double *x) { sim3_update(S, x, pr.fix_scale); }

    int classify(int mark) {
        int bad = 0;
        for (int i = 0; i < pr.n; ++i) {
            if (flags[i]) continue;
            if (pr.chi12[i] > pr.th2 || pr.chi21[i] > pr.th2) {
                flags[i] = (uint8_t)mark;
                ++bad;
            }
        }
        return bad;
    }
};

Sim3 load(const orbx_sim3 *s) {
    Sim3 S;
    std::memcpy(&S, s, sizeof(S));
    return S;
}

}  // namespace

extern "C" {

int sim3_host_optimize(const orbx_sim3 *S12, const orbx_sim3_camera *cam1, const orbx_sim3_camera *cam2,
                       const orbx_sim3_corr *corr, int n, float th2, int fix_scale, orbx_sim3 *S12_out,
                       uint8_t *removed, double *chi2_12, double *chi2_21, int *n_inliers, int *iterations) {
    HostExec ex;
    ex.pr.corr = corr;
    ex.pr.n = n;
    ex.pr.flag = removed;
    ex.pr.sense = false;
    ex.pr.chi12 = chi2_12;
    ex.pr.chi21 = chi2_21;
    ex.pr.c1 = sim3_cam(*cam1);
    ex.pr.c2 = sim3_cam(*cam2);
    sim3_problem_thresholds(ex.pr, th2);
    ex.pr.fix_scale = fix_scale;
    ex.pr.robust = true;
    ex.flags = removed;
    for (int i = 0; i < n; ++i) {
        removed[i] = 0;
        chi2_12[i] = 0;
        chi2_21[i] = 0;
    }
    Sim3 out;
    sim3_optimize(ex, load(S12), n, out, *n_inliers, iterations);
    std::memcpy(S12_out, &out, sizeof(out));
    return 0;
}

int sim3_host_step(const orbx_sim3 *S12, const orbx_sim3_camera *cam1, const orbx_sim3_camera *cam2,
                   const orbx_sim3_corr *corr, int n, float th2, int fix_scale, const uint8_t *active, int robust,
                   double lambda, double *H_out, double *b_out, double *x_out, double *chi2_out, int *solved) {
    std::vector<double> c12(n + 1), c21(n + 1);
    HostExec ex;
    ex.pr.corr = corr;
    ex.pr.n = n;
    ex.pr.flag = active;
    ex.pr.sense = true;
    ex.pr.chi12 = c12.data();
    ex.pr.chi21 = c21.data();
    ex.pr.c1 = sim3_cam(*cam1);
    ex.pr.c2 = sim3_cam(*cam2);
    sim3_problem_thresholds(ex.pr, th2);
    ex.pr.fix_scale = fix_scale;
    ex.pr.robust = robust != 0;
    ex.flags = nullptr;
    ex.build(load(S12), H_out, b_out, chi2_out);
    double x[7];
    const bool ok = lm_solve<7>(H_out, b_out, lambda, x);
    for (int j = 0; j < 7; ++j) x_out[j] = ok ? x[j] : 0.0;
    *solved = ok;
    return 0;
}

int sim3_host_update(const orbx_sim3 *S, const double *x, int count, int fix_scale, orbx_sim3 *S_out) {
    for (int k = 0; k < count; ++k) {
        Sim3 s = load(S + k);
        sim3_update(s, x + 7 * k, fix_scale);
        std::memcpy(S_out + k, &s, sizeof(s));
    }
    return 0;
}

// Sim3(u) itself and entry k of the perturbation table (the test that the table's constants are sim3_exp's values)
void sim3_host_exp(const double *u, orbx_sim3 *out) {
    Sim3 s;
    sim3_exp(u, s);
    std::memcpy(out, &s, sizeof(s));
}

void sim3_host_perturbation(int k, int fix_scale, orbx_sim3 *out) {
    Sim3 s;
    sim3_perturbation(k, fix_scale, s);
    std::memcpy(out, &s, sizeof(s));
}

}  // extern "C"
