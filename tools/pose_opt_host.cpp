// pose_opt_host — Optimizer::PoseOptimization as a scalar host program: the algorithm of csrc/k_poseopt.hip (tests/_poseopt_ref.py is the
// normative text), statement for statement, for tools/time_pose_opt.py (g++ -O3 -ffp-contract=off).  With -DPO_TREE every sum over the edges
// is the perfect binary tree of P5 and the answers equal the device's bit for bit; without it the sums run in feature order, as g2o's do -
// the faster form on a host, and the one that is timed.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {
const double EXP_A[16] = {0x1.0000000000000p+0, -0x1.5555555555555p-3, 0x1.1111111111111p-7, -0x1.a01a01a01a01ap-13, 0x1.71de3a556c734p-19,
                          -0x1.ae64567f544e4p-26, 0x1.6124613a86d09p-33, -0x1.ae7f3e733b81fp-41, 0x1.952c77030ad4ap-49, -0x1.2f49b46814157p-57,
                          0x1.71b8ef6dcf572p-66, -0x1.761b41316381ap-75, 0x1.3f3ccdd165fa9p-84, -0x1.d1ab1c2dccea3p-94, 0x1.259f98b4358adp-103,
                          -0x1.434d2e783f5bcp-113};
const double EXP_B[16] = {0x1.0000000000000p-1, -0x1.5555555555555p-5, 0x1.6c16c16c16c17p-10, -0x1.a01a01a01a01ap-16, 0x1.27e4fb7789f5cp-22,
                          -0x1.1eed8eff8d898p-29, 0x1.93974a8c07c9dp-37, -0x1.ae7f3e733b81fp-45, 0x1.6827863b97d97p-53, -0x1.e542ba4020225p-62,
                          0x1.0ce396db7f853p-70, -0x1.f2cf01972f578p-80, 0x1.88e85fc6a4e5ap-89, -0x1.0a18a2635085dp-98, 0x1.3932c5047d60ep-108,
                          -0x1.434d2e783f5bcp-118};
const double EXP_C[16] = {0x1.5555555555555p-3, -0x1.1111111111111p-7, 0x1.a01a01a01a01ap-13, -0x1.71de3a556c734p-19, 0x1.ae64567f544e4p-26,
                          -0x1.6124613a86d09p-33, 0x1.ae7f3e733b81fp-41, -0x1.952c77030ad4ap-49, 0x1.2f49b46814157p-57, -0x1.71b8ef6dcf572p-66,
                          0x1.761b41316381ap-75, -0x1.3f3ccdd165fa9p-84, 0x1.d1ab1c2dccea3p-94, -0x1.259f98b4358adp-103, 0x1.434d2e783f5bcp-113,
                          -0x1.3981254dd0d52p-123};
const double PI2 = 0x1.3bd3cc9be45dep+3, DELTA_MONO = 0x1.394ca80000000p+1, DELTA_STEREO = 0x1.65d4000000000p+1;
const int NV = 28;

struct Edge {
    double X, Y, Z, ox, oy, our, inf;
    bool edge, stereo, flagged;
};
struct Cam {
    double fx, fy, cx, cy, bf;
};

double horner(const double *c, double t2) {
    double r = c[15];
    for (int k = 14; k >= 0; --k) r = r * t2 + c[k];
    return r;
}

double error(const Edge &E, const Cam &C, const double *R, const double *t, double &x, double &y, double &z, double *e) {
    x = (R[0] * E.X + (R[1] * E.Y + R[2] * E.Z)) + t[0];
    y = (R[3] * E.X + (R[4] * E.Y + R[5] * E.Z)) + t[1];
    z = (R[6] * E.X + (R[7] * E.Y + R[8] * E.Z)) + t[2];
    const double px = C.fx * (x / z) + C.cx, py = C.fy * (y / z) + C.cy;
    e[0] = E.ox - px;
    e[1] = E.oy - py;
    e[2] = E.stereo ? E.our - (px - C.bf / z) : 0.0;
    const double c2 = E.stereo ? e[2] * (E.inf * e[2]) : 0.0;
    return e[0] * (E.inf * e[0]) + (e[1] * (E.inf * e[1]) + c2);
}

double huber(double chi2, bool stereo, bool robust, double &rho1) {
    if (!robust) {
        rho1 = 1.0;
        return chi2;
    }
    const double delta = stereo ? DELTA_STEREO : DELTA_MONO, dsqr = delta * delta, s = std::sqrt(chi2);
    const bool inl = chi2 <= dsqr;
    rho1 = inl ? 1.0 : delta / s;
    return inl ? chi2 : (2.0 * s) * delta - dsqr;
}

void linearise(const Edge &E, const Cam &C, const double *R, const double *t, bool robust, double *out) {
    double x, y, z, e[3], rho1;
    const double chi2 = error(E, C, R, t, x, y, z, e);
    out[27] = huber(chi2, E.stereo, robust, rho1);
    const double inf = E.inf, invz = 1.0 / z, invz2 = invz * invz, fx = C.fx, fy = C.fy, bf = C.bf;
    double J[3][6];
    J[0][0] = ((x * y) * invz2) * fx;
    J[0][1] = -((1.0 + (x * x) * invz2) * fx);
    J[0][2] = (y * invz) * fx;
    J[0][3] = -(invz * fx);
    J[0][4] = 0.0;
    J[0][5] = (x * invz2) * fx;
    J[1][0] = (1.0 + (y * y) * invz2) * fy;
    J[1][1] = -(((x * y) * invz2) * fy);
    J[1][2] = -((x * invz) * fy);
    J[1][3] = 0.0;
    J[1][4] = -(invz * fy);
    J[1][5] = (y * invz2) * fy;
    J[2][0] = J[0][0] - (bf * y) * invz2;
    J[2][1] = J[0][1] + (bf * x) * invz2;
    J[2][2] = J[0][2];
    J[2][3] = J[0][3];
    J[2][4] = 0.0;
    J[2][5] = J[0][5] - bf * invz2;
    const double w = robust ? rho1 * inf : inf;
    double g[3];
    for (int k = 0; k < 3; ++k) {
        g[k] = -(inf * e[k]);
        if (robust) g[k] = rho1 * g[k];
    }
    int o = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) {
            const double a2 = E.stereo ? J[2][i] * (w * J[2][j]) : 0.0;
            out[o++] = J[0][i] * (w * J[0][j]) + (J[1][i] * (w * J[1][j]) + a2);
        }
    for (int j = 0; j < 6; ++j) {
        const double a2 = E.stereo ? J[2][j] * g[2] : 0.0;
        out[21 + j] = J[0][j] * g[0] + (J[1][j] * g[1] + a2);
    }
}

inline int hidx(int i, int j) { return i * 6 - (i * (i - 1)) / 2 + (j - i); }

bool solve6(const double *S, double lam, double *x) {
    double L[6][6];
    for (int j = 0; j < 6; ++j) {
        double s = S[hidx(j, j)] + lam;
        for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k];
        if (!(s > 0.0 && std::isfinite(s))) return false;
        L[j][j] = std::sqrt(s);
        for (int i = j + 1; i < 6; ++i) {
            double q = S[hidx(j, i)];
            for (int k = 0; k < j; ++k) q = q - L[i][k] * L[j][k];
            L[i][j] = q / L[j][j];
        }
    }
    double y[6];
    for (int i = 0; i < 6; ++i) {
        double s = S[21 + i];
        for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
        for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * x[k];
        x[i] = s / L[i][i];
    }
    return true;
}

bool exp_step(const double *R, const double *t, const double *x, double *Rn, double *tn) {
    const double w0 = x[0], w1 = x[1], w2 = x[2];
    const double t2 = w0 * w0 + (w1 * w1 + w2 * w2);
    if (t2 > PI2) return false;
    const double A = horner(EXP_A, t2), B = horner(EXP_B, t2), Cc = horner(EXP_C, t2);
    const double W[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
    const double W2[3][3] = {{-(w1 * w1 + w2 * w2), w0 * w1, w0 * w2}, {w0 * w1, -(w0 * w0 + w2 * w2), w1 * w2}, {w0 * w2, w1 * w2, -(w0 * w0 + w1 * w1)}};
    double dR[3][3], V[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            dR[i][j] = i == j ? 1.0 + B * W2[i][j] : A * W[i][j] + B * W2[i][j];
            V[i][j] = i == j ? 1.0 + Cc * W2[i][j] : B * W[i][j] + Cc * W2[i][j];
        }
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) Rn[3 * i + j] = dR[i][0] * R[j] + (dR[i][1] * R[3 + j] + dR[i][2] * R[6 + j]);
        tn[i] = (dR[i][0] * t[0] + (dR[i][1] * t[1] + dR[i][2] * t[2])) + (V[i][0] * x[3] + (V[i][1] * x[4] + V[i][2] * x[5]));
    }
    return true;
}

// the sums of nv values per feature: leaf(i, out) fills out[0 .. nv) for an active feature
struct Sums {
    int n, P;
    std::vector<double> buf;
    explicit Sums(int n_) : n(n_), P(1) {
        while (P < (n > 1 ? n : 1)) P *= 2;
#ifdef PO_TREE
        buf.resize((size_t)P * NV);
#endif
    }
    template <class Active, class Leaf>
    void run(int nv, Active active, Leaf leaf, double *tot) {
        double v[NV];
#ifdef PO_TREE
        for (int i = 0; i < P; ++i) {
            const bool a = i < n && active(i);
            if (a) leaf(i, v);
            for (int k = 0; k < nv; ++k) buf[(size_t)k * P + i] = a ? v[k] + 0.0 : 0.0;
        }
        for (int k = 0; k < nv; ++k) {
            double *b = buf.data() + (size_t)k * P;
            for (int w = P; w > 1; w /= 2)
                for (int i = 0; i < w / 2; ++i) b[i] = b[2 * i] + b[2 * i + 1];
            tot[k] = b[0];
        }
#else
        for (int k = 0; k < nv; ++k) tot[k] = 0.0;
        for (int i = 0; i < n; ++i)
            if (active(i)) {
                leaf(i, v);
                for (int k = 0; k < nv; ++k) tot[k] += v[k];
            }
#endif
    }
};
}  // namespace

// pose12: Rcw row-major, tcw.  ints: rounds, n_edges, iterations[4], trials[4]; dbls: chi2[4], lambda[4].  Returns nInitialCorrespondences - nBad
extern "C" int pose_opt_host(int n, const float *x, const float *y, const float *ur, const float *inf, const int32_t *pts, const float *store_pos,
                             const uint8_t *store_set, int cap, const float *cam5, const float *pose12, float *pose12_out, uint8_t *outlier,
                             int32_t *ints, double *dbls) {
    const Cam C = {cam5[0], cam5[1], cam5[2], cam5[3], cam5[4]};
    std::vector<Edge> E((size_t)n);
    int n_edges = 0;
    for (int i = 0; i < n; ++i) {
        Edge e{};
        const int id = pts[i];
        if (id >= 0 && id < cap && store_set[id]) {
            e.X = store_pos[3 * id]; e.Y = store_pos[3 * id + 1]; e.Z = store_pos[3 * id + 2];
            e.ox = x[i]; e.oy = y[i]; e.our = ur[i]; e.inf = inf[i];
            e.edge = true;
            e.stereo = !(ur[i] < 0.0f);
            ++n_edges;
        }
        E[(size_t)i] = e;
    }
    double R[9], t[3];
    for (int k = 0; k < 9; ++k) R[k] = pose12[k];
    for (int k = 0; k < 3; ++k) t[k] = pose12[9 + k];
    std::memset(ints, 0, 10 * sizeof(int32_t));
    std::memset(dbls, 0, 8 * sizeof(double));
    std::memset(outlier, 0, (size_t)n);
    int rounds = 0, n_bad = 0;
    Sums sums(n);
    auto active = [&](int i) { return E[(size_t)i].edge && !E[(size_t)i].flagged; };
    if (n_edges >= 3) {
        for (int r = 0; r < 4; ++r) {
            const bool robust = r < 3;
            for (int k = 0; k < 9; ++k) R[k] = pose12[k];
            for (int k = 0; k < 3; ++k) t[k] = pose12[9 + k];
            int n_active = 0;
            for (int i = 0; i < n; ++i) n_active += active(i);
            int iterations = 0, trials = 0;
            double cur = 0.0, lam = 0.0, ni = 2.0;
            if (n_active > 0) {
                for (int it = 0; it < 10; ++it) {
                    double tot[NV];
                    sums.run(NV, active, [&](int i, double *v) { linearise(E[(size_t)i], C, R, t, robust, v); }, tot);
                    cur = tot[27];
                    if (it == 0) {
                        double m = std::fabs(tot[hidx(0, 0)]);
                        for (int j = 1; j < 6; ++j) {
                            const double a = std::fabs(tot[hidx(j, j)]);
                            m = a > m ? a : m;
                        }
                        lam = 1e-5 * m;
                        ni = 2.0;
                    }
                    ++iterations;
                    double rho = 0.0;
                    int qmax = 0;
                    do {
                        ++trials;
                        double xs[6], Rn[9], tn[3];
                        bool ok = solve6(tot, lam, xs);
                        if (ok) ok = exp_step(R, t, xs, Rn, tn);
                        bool accepted = false;
                        double temp = 0.0;
                        if (ok) {
                            sums.run(1, active, [&](int i, double *v) {
                                double px, py, pz, e[3], rho1;
                                v[0] = huber(error(E[(size_t)i], C, Rn, tn, px, py, pz, e), E[(size_t)i].stereo, robust, rho1);
                            }, &temp);
                            double scale = 0.0;
                            for (int j = 0; j < 6; ++j) scale = scale + xs[j] * (lam * xs[j] + tot[21 + j]);
                            scale = scale + 1e-3;
                            rho = (cur - temp) / scale;
                            accepted = rho > 0.0 && std::isfinite(temp);
                        } else {
                            rho = -1.0;
                        }
                        if (accepted) {
                            const double q = 2.0 * rho - 1.0;
                            double alpha = 1.0 - (q * q) * q;
                            const double up = 2.0 / 3.0, low = 1.0 / 3.0;
                            alpha = up < alpha ? up : alpha;
                            lam = lam * (low < alpha ? alpha : low);
                            ni = 2.0;
                            cur = temp;
                            std::memcpy(R, Rn, sizeof(R));
                            std::memcpy(t, tn, sizeof(t));
                        } else {
                            lam = lam * ni;
                            ni = ni * 2.0;
                        }
                        ++qmax;
                    } while (rho < 0.0 && qmax < 10);
                    if (qmax == 10 || rho == 0.0) break;
                }
            }
            n_bad = 0;
            for (int i = 0; i < n; ++i) {
                Edge &e = E[(size_t)i];
                if (!e.edge) continue;
                double px, py, pz, er[3];
                const double chi2 = error(e, C, R, t, px, py, pz, er);
                e.flagged = !std::isfinite(chi2) || (float)chi2 > (e.stereo ? 7.815f : 5.991f);
                n_bad += e.flagged;
            }
            ints[2 + r] = iterations;
            ints[6 + r] = trials;
            dbls[r] = cur;
            dbls[4 + r] = lam;
            rounds = r + 1;
            if (n_edges < 10) break;
        }
    }
    for (int k = 0; k < 9; ++k) pose12_out[k] = (float)R[k];
    for (int k = 0; k < 3; ++k) pose12_out[9 + k] = (float)t[k];
    for (int i = 0; i < n; ++i) outlier[i] = E[(size_t)i].flagged;
    ints[0] = rounds;
    ints[1] = n_edges;
    return rounds ? n_edges - n_bad : 0;
}
