// sim3opt_host.cpp — Optimizer::OptimizeSim3 as tests/_sim3opt_ref.py restates it, as a scalar host program: what tools/time_sim3opt.py
// times the device against and compares its answers with, and what tests/test_sim3opt_host_cpu.py holds to the restatement bit for bit.
//
//   g++ -O3 -ffp-contract=off -std=c++17 -I anyfeature-vslam_amd/csrc -shared -fPIC tools/sim3opt_host.cpp -o sim3opt_host.so
//   g++ -O1 -g -ffp-contract=off -std=c++17 -fsanitize=address,undefined -DSIM3OPT_HOST_MAIN -I anyfeature-vslam_amd/csrc tools/sim3opt_host.cpp -o sim3opt_host && ./sim3opt_host
//
// The scalar arithmetic (the exponential, the two edges, Huber, the 36 terms of a correspondence, the 7 x 7 solve, the Levenberg
// verdict) is csrc/afv_sim3opt_math.h, the text the kernel compiles; the edge set, the sums (O5), optimize() and the classifications
// are written here on their own, sequentially.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "afv_sim3opt_math.h"

namespace {

struct Problem {
    std::vector<SoEdge> edges;
    std::vector<int> index1;
    std::vector<uint8_t> active;
    SoCam K1, K2;
    double delta, th2;
    bool fix_scale;
};

struct Sum36 {  // O5: 64 partial sums per value, then the halving tree
    double p[36][64];
    Sum36() { std::memset(p, 0, sizeof(p)); }
    void add(int k, const double (&term)[36]) {
        for (int q = 0; q < 36; ++q) p[q][k & 63] = p[q][k & 63] + term[q];
    }
    void tree(double (&out)[36]) {
        for (int q = 0; q < 36; ++q) {
            for (int s = 32; s >= 1; s >>= 1)
                for (int l = 0; l < s; ++l) p[q][l] = p[q][l] + p[q][l + s];
            out[q] = p[q][0];
        }
    }
};

float row(const float *R, const float *t, int r, const float *X) { return (R[3 * r] * X[0] + (R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2])) + t[r]; }

double robust_chi2(const Problem &P, const SoPair &E) {
    double p[64];
    for (double &v : p) v = 0.0;
    for (size_t k = 0; k < P.edges.size(); ++k)
        if (P.active[k]) p[k & 63] = p[k & 63] + so_edge_robust(E, P.K1, P.K2, P.edges[k], P.delta);
    for (int s = 32; s >= 1; s >>= 1)
        for (int l = 0; l < s; ++l) p[l] = p[l] + p[l + s];
    return p[0];
}

void linearise(const Problem &P, const SoPair &E, double (&acc)[36]) {
    SoPair pert[14];  // BaseBinaryEdge::linearizeOplus: 2 d = +delta e_d, 2 d + 1 = -delta e_d
    for (int p = 0; p < 14; ++p) {
        double u[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        u[p >> 1] = (p & 1) ? -SO_DELTA : SO_DELTA;
        (void)so_step(E.f, u, P.fix_scale, pert[p]);
    }
    const double scalar = 1.0 / (2.0 * SO_DELTA);
    Sum36 sum;
    for (size_t k = 0; k < P.edges.size(); ++k) {
        if (!P.active[k]) continue;
        const SoEdge &g = P.edges[k];
        double e12[2], e21[2], J12[2][7], J21[2][7];
        so_edge_errors(E, P.K1, P.K2, g, e12, e21);
        for (int d = 0; d < 7; ++d) {
            double p12[2], p21[2], m12[2], m21[2];
            so_edge_errors(pert[2 * d], P.K1, P.K2, g, p12, p21);
            so_edge_errors(pert[2 * d + 1], P.K1, P.K2, g, m12, m21);
            for (int r = 0; r < 2; ++r) {
                J12[r][d] = scalar * (p12[r] - m12[r]);
                J21[r][d] = scalar * (p21[r] - m21[r]);
            }
        }
        double term[36];
        so_edge_terms(e12, e21, J12, J21, g.inf1, g.inf2, P.delta, term);
        sum.add((int)k, term);
    }
    sum.tree(acc);
}

struct Stage {
    int iterations = 0, trials = 0;
    double chi2 = 0.0, lambda = 0.0;
};

Stage optimize(const Problem &P, SoPair &E, int n_active, int iterations) {
    Stage S;
    if (n_active == 0) return S;  // O7
    double lam = 0.0, ni = 2.0, cur = 0.0;
    for (int it = 0; it < iterations; ++it) {
        double acc[36], Hu[28], b[7];
        linearise(P, E, acc);
        for (int q = 0; q < 28; ++q) Hu[q] = acc[q];
        for (int q = 0; q < 7; ++q) b[q] = acc[28 + q];
        cur = acc[35];
        if (it == 0) {
            lam = so_lambda_init(Hu);
            ni = 2.0;
        }
        ++S.iterations;
        double rho = 0.0;
        int qmax = 0;
        do {
            ++S.trials;
            double x[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            SoPair st = E;
            bool failed = !so_solve7(Hu, b, lam, x);
            if (!failed) failed = !so_step(E.f, x, P.fix_scale, st);
            const double temp = failed ? 0.0 : robust_chi2(P, st);
            const SoTrial T = so_judge(failed, cur, temp, x, b, lam, ni);
            rho = T.rho;
            if (T.accepted) {
                cur = temp;
                E = st;
            }
            ++qmax;
        } while (rho < 0.0 && qmax < SO_MAX_TRIALS);
        if (qmax == SO_MAX_TRIALS || rho == 0.0) break;
    }
    S.chi2 = cur;
    S.lambda = lam;
    return S;
}

}  // namespace

// nc jobs that share keyframe 1 (n1 features: x1, y1, inf1, mp1) and the store (pos [P][3], flags [P]: 1 = set, 2 = bad); per job c:
// cams[c][32] = (Rcw[9], tcw[3], fx, fy, cx, cy) of keyframe 1, then of keyframe 2; start[c][13] = R12, t12, s12; th2[c]; fix_scale[c];
// x2 / y2 / inf2 [c][n2]; mp2 / idx2 [c][n1].  Out per job: ints[c][9] = n_in, n_corr, n_bad, more_iterations, early, iterations[2],
// trials[2]; doubles[c][17] = R12[9], t12[3], s12, chi2[2], lambda[2]; state[c][n1].
extern "C" void sim3opt_host(int nc, int n1, int n2, const float *cams, const float *start, const float *th2, const int32_t *fix_scale, const float *pos,
                             const uint8_t *flags, const float *x1, const float *y1, const float *inf1, const int32_t *mp1, const float *x2,
                             const float *y2, const float *inf2, const int32_t *mp2, const int32_t *idx2, int32_t *ints, double *doubles,
                             uint8_t *state) {
    for (int c = 0; c < nc; ++c) {
        const float *cam1 = cams + (size_t)c * 32, *cam2 = cam1 + 16, *S0 = start + (size_t)c * 13;
        const size_t r1 = (size_t)c * n1, r2 = (size_t)c * n2;
        uint8_t *st = state + r1;
        Problem P;
        P.K1 = SoCam{(double)cam1[12], (double)cam1[13], (double)cam1[14], (double)cam1[15]};
        P.K2 = SoCam{(double)cam2[12], (double)cam2[13], (double)cam2[14], (double)cam2[15]};
        P.delta = (double)sqrtf(th2[c]);
        P.th2 = (double)th2[c];
        P.fix_scale = fix_scale[c] != 0;
        for (int i = 0; i < n1; ++i) {  // the edge set (:1084-1163)
            const int p1 = mp1[i], p2 = mp2[r1 + i], k2 = idx2[r1 + i];
            st[i] = p2 < 0 ? 0 : 1;
            if (p2 < 0 || p1 < 0) continue;
            if (!(flags[p1] & 1) || (flags[p1] & 2) || !(flags[p2] & 1) || (flags[p2] & 2) || k2 < 0) continue;
            SoEdge g;
            for (int r = 0; r < 3; ++r) {
                g.p1[r] = (double)row(cam1, cam1 + 9, r, pos + 3 * (size_t)p1);
                g.p2[r] = (double)row(cam2, cam2 + 9, r, pos + 3 * (size_t)p2);
            }
            g.obs1[0] = (double)x1[i]; g.obs1[1] = (double)y1[i];
            g.obs2[0] = (double)x2[r2 + k2]; g.obs2[1] = (double)y2[r2 + k2];
            g.inf1 = (double)inf1[i];
            g.inf2 = (double)inf2[r2 + k2];
            P.edges.push_back(g);
            P.index1.push_back(i);
            P.active.push_back(1);
            st[i] = 2;
        }
        const int n = (int)P.edges.size();
        SoPair E0;
        for (int k = 0; k < 9; ++k) E0.f.R[k] = (double)S0[k];
        for (int k = 0; k < 3; ++k) E0.f.t[k] = (double)S0[9 + k];
        E0.f.s = (double)S0[12];
        so_inverse(E0.f, E0.i);
        SoPair E = E0;
        const Stage A = optimize(P, E, n, 5);
        int n_bad = 0;
        for (int k = 0; k < n; ++k)
            if (so_edge_outlier(E, P.K1, P.K2, P.edges[k], P.th2)) {
                P.active[k] = 0;
                st[P.index1[k]] = 3;
                ++n_bad;
            }
        const int more = n_bad > 0 ? 10 : 5;
        const bool early = n - n_bad < SO_MIN_CORRESPONDENCES;
        Stage B;
        int n_in = 0;
        if (!early) {
            B = optimize(P, E, n - n_bad, more);
            for (int k = 0; k < n; ++k) {
                if (!P.active[k]) continue;
                if (so_edge_outlier(E, P.K1, P.K2, P.edges[k], P.th2)) st[P.index1[k]] = 4;
                else ++n_in;
            }
        }
        const SoEst &out = early ? E0.f : E.f;
        int32_t *I = ints + (size_t)c * 9;
        I[0] = n_in; I[1] = n; I[2] = n_bad; I[3] = more; I[4] = early ? 1 : 0;
        I[5] = A.iterations; I[6] = B.iterations; I[7] = A.trials; I[8] = B.trials;
        double *D = doubles + (size_t)c * 17;
        for (int k = 0; k < 9; ++k) D[k] = out.R[k];
        for (int k = 0; k < 3; ++k) D[9 + k] = out.t[k];
        D[12] = out.s;
        D[13] = A.chi2; D[14] = B.chi2; D[15] = A.lambda; D[16] = B.lambda;
    }
}

#ifdef SIM3OPT_HOST_MAIN
// a stand-alone run on a small built-in world (for sanitizer builds): 24 points seen by two identity cameras, a start 2 % off in scale
int main() {
    const int n = 24;
    std::vector<float> cams(32, 0.0f), start(13, 0.0f), pos(6 * n), x1(n), y1(n), inf(n, 1.0f), x2(n), y2(n);
    std::vector<uint8_t> flags(2 * n, 1), state(n);
    std::vector<int32_t> mp1(n), mp2(n), idx2(n);
    for (int c = 0; c < 2; ++c) {
        float *cam = cams.data() + 16 * c;
        cam[0] = cam[4] = cam[8] = 1.0f;
        cam[12] = cam[13] = 500.0f; cam[14] = 320.0f; cam[15] = 240.0f;
    }
    start[0] = start[4] = start[8] = 1.0f;
    start[9] = 0.26f; start[12] = 1.02f;
    unsigned r = 12345u;
    auto rnd = [&r] { r = r * 1664525u + 1013904223u; return (float)(r >> 8) / 16777216.0f; };
    for (int i = 0; i < n; ++i) {
        float *a = pos.data() + 3 * i, *b = pos.data() + 3 * (n + i);
        a[0] = 4.0f * rnd() - 2.0f; a[1] = 3.0f * rnd() - 1.5f; a[2] = 3.0f + 6.0f * rnd();
        b[0] = a[0] - 0.25f; b[1] = a[1]; b[2] = a[2];  // map 2 = map 1 - (0.25, 0, 0)
        x1[i] = 500.0f * a[0] / a[2] + 320.0f; y1[i] = 500.0f * a[1] / a[2] + 240.0f;
        x2[i] = 500.0f * b[0] / b[2] + 320.0f; y2[i] = 500.0f * b[1] / b[2] + 240.0f;
        mp1[i] = i; mp2[i] = n + i; idx2[i] = i;
    }
    const float th2 = 10.0f;
    const int32_t fix = 0;
    int32_t ints[9];
    double doubles[17];
    sim3opt_host(1, n, n, cams.data(), start.data(), &th2, &fix, pos.data(), flags.data(), x1.data(), y1.data(), inf.data(), mp1.data(), x2.data(),
                 y2.data(), inf.data(), mp2.data(), idx2.data(), ints, doubles, state.data());
    std::printf("n_in %d n_corr %d n_bad %d early %d s12 %.17g t12 %.17g %.17g %.17g chi2 %.6g %.6g\n", ints[0], ints[1], ints[2], ints[4], doubles[12],
                doubles[9], doubles[10], doubles[11], doubles[13], doubles[14]);
    return ints[0] == n ? 0 : 1;
}
#endif
