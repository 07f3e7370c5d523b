// Host run of the GICP control step (xchu_slam_amd/csrc/ndt_gicp.h: the text the last workgroup of k_gicp_pairs /
// k_gicp_eval runs) over a dumped pair set, with a host evaluator in place of k_gicp_eval: the 13 sums in pair order.
// Input (argv[1]): f64 values — m, max_inner, rot_eps, trans_eps, guess[16], transformation_[16] (column-major), then per
// pair p[3], q[3], guess*p[3], M[9] (rows).  Output: one line per trial point ("x" and six %a values), then the
// solve's status, inner iterations, evaluations, f, delta, the convergence state and transformation_.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../xchu_slam_amd/csrc/ndt_gicp.h"

using namespace ndt;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) return 2;
    std::vector<double> v;
    double buf[1024];
    size_t n;
    while ((n = std::fread(buf, sizeof(double), 1024, fp)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(fp);
    if (v.size() < 36) return 2;
    const int m = (int)v[0];
    if (v.size() != 36 + (size_t)18 * m) return 2;
    static GicpState st;
    static GicpRecordDev hist[kGicpMaxHistory];
    st.max_inner = (int)v[1];
    st.rot_eps = v[2];
    st.trans_eps = v[3];
    st.max_iter = 1 << 30;
    for (int k = 0; k < 16; ++k) { st.guess[k] = (float)v[4 + k]; st.trans[k] = (float)v[20 + k]; st.prev[k] = st.trans[k]; }
    gicp_set_rtg(&st);
    st.phase = GICP_PAIRS;
    gicp_after_pairs(&st, hist, m);
    const double* P = v.data() + 36;
    while (st.phase == GICP_EVAL) {
        std::printf("x %a %a %a %a %a %a\n", st.min.x[0], st.min.x[1], st.min.x[2], st.min.x[3], st.min.x[4], st.min.x[5]);
        const float* T = st.T_trial;
        double S[kGicpSums];
        for (int k = 0; k < kGicpSums; ++k) S[k] = 0.0;
        for (int i = 0; i < m; ++i) {
            const double* r = P + (size_t)18 * i;
            const float p[3] = {(float)r[0], (float)r[1], (float)r[2]}, q[3] = {(float)r[3], (float)r[4], (float)r[5]};
            const double* M = r + 9;
            float pp[3];
            for (int a = 0; a < 3; ++a) pp[a] = ((T[a] * p[0] + T[a + 4] * p[1]) + T[a + 8] * p[2]) + T[a + 12];
            const double res[3] = {(double)(pp[0] - q[0]), (double)(pp[1] - q[1]), (double)(pp[2] - q[2])};
            double tmp[3];
            for (int a = 0; a < 3; ++a) tmp[a] = (M[3 * a] * res[0] + M[3 * a + 1] * res[1]) + M[3 * a + 2] * res[2];
            S[0] += (res[0] * tmp[0] + res[1] * tmp[1]) + res[2] * tmp[2];
            for (int a = 0; a < 3; ++a) S[1 + a] += tmp[a];
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) S[4 + 3 * a + b] += r[6 + a] * tmp[b];
        }
        gicp_after_eval(&st, hist, S);
    }
    const GicpRecordDev& h = hist[0];
    std::printf("end status %d inner %d evals %d f %a delta %a state %d phase %d\n", h.status, h.inner, h.evals, h.f, h.delta,
                h.conv_state, st.phase);
    std::printf("T");
    for (int k = 0; k < 16; ++k) std::printf(" %a", (double)st.trans[k]);
    std::printf("\n");
    return 0;
}
