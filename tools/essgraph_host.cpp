// essgraph_host.cpp — OptimizeEssentialGraph as tests/_essgraph_ref.py restates it, as a scalar host program: the work of every lane of
// csrc/k_essgraph.hip (csrc/afv_essgraph_math.h, shared text) called in plain loops, the plan of csrc/afv_essgraph_plan.h (the same the
// library builds), the 64-partial trees, the walk over the block columns and the driver written out.  It is the route a host has
// without the device and the bit-equal second witness: tools/time_essgraph.py times it against the device and
// tests/test_essgraph_host_cpu.py holds it to the restatement bit for bit.  Build: g++ -O3 -ffp-contract=off -std=c++17 -I
// anyfeature-vslam_amd/csrc -shared -fPIC (the tests), or -DESSGRAPH_HOST_MAIN for a stand-alone program that reads a scene file
// (int32 nk, fixed, ne, iterations, fix_scale, np; double lambda_init; S_init [nk][13]; v0 [ne]; v1 [ne]; meas [ne][13]; then np points:
// pos [np][3] float, ok [np] bytes, ref [np] int32) and prints the answer - the form the sanitizer run takes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "afv_essgraph_math.h"
#include "afv_essgraph_plan.h"

namespace {

double tree64(double (&p)[64]) {  // p[l] += p[l + s], s = 32 .. 1
    for (int s = 32; s >= 1; s >>= 1)
        for (int l = 0; l < s; ++l) p[l] = p[l] + p[l + s];
    return p[0];
}

struct Host {
    EgView V{};
    EgStatus st{};
    EgPlan P;
    std::vector<double> S, pert, perr, term, Hd, Aoff, L, rhs, chi_trial;
    std::vector<uint8_t> e_bad, v_fail;
    int32_t solve_fail = 0;
};

void linearise(Host &H, double lambda_init) {
    const EgView &V = H.V;
    for (int k = 0; k < V.nk; ++k)
        for (int q = 0; q < 14; ++q) eg_perturb(V, k, q);
    for (int e = 0; e < V.ne; ++e)
        for (int p = 0; p < EG_NP; ++p) eg_edge_perr(V, e, p);
    for (int e = 0; e < V.ne; ++e)
        for (int q = 0; q < EG_NT; ++q) eg_edge_term(V, e, q);
    for (int i = 0; i < V.nf; ++i)
        for (int q = 0; q < 35; ++q) {
            double part[64];
            for (int l = 0; l < 64; ++l) part[l] = eg_vertex_partial(V, i, q, l);
            V.Hd[(size_t)i * 35 + q] = tree64(part);
        }
    for (int q = 0; q < V.nob; ++q)
        for (int t = 0; t < 49; ++t) V.Aoff[(size_t)q * 49 + t] = eg_offdiag_entry(V, q, t / 7, t % 7);
    double c[64];
    bool bad = false;
    for (int l = 0; l < 64; ++l) c[l] = eg_edge_partial(V, V.term + 119, EG_NT, l);
    for (int e = 0; e < V.ne; ++e) bad = bad || V.e_bad[e];
    eg_begin(*V.st, tree64(c), bad, lambda_init);
}

// G1: block column j is finished before column j + 1; then the two substitutions
bool factor_solve(const EgView &V) {
    for (int b = 0; b < V.nb; ++b)
        for (int t = 0; t < 49; ++t) eg_load_entry(V, b, t);
    for (int i = 0; i < 7 * V.nf; ++i) V.rhs[i] = V.Hd[(size_t)(i / 7) * 35 + 28 + i % 7];
    for (int j = 0; j < V.nf; ++j) {
        const int b0 = V.col_ptr[j], b1 = V.col_ptr[j + 1];
        if (!eg_chol7(V.L + (size_t)b0 * 49)) return false;
        for (int b = b0 + 1; b < b1; ++b)
            for (int a = 0; a < 7; ++a) eg_trsm_row(V.L + (size_t)b0 * 49, V.L + (size_t)b * 49, a);
        for (int u = V.upd_ptr[j]; u < V.upd_ptr[j + 1]; ++u)
            for (int t = 0; t < 49; ++t)
                eg_update_entry(V.L + (size_t)V.upd[3 * u] * 49, V.L + (size_t)V.upd[3 * u + 1] * 49, V.L + (size_t)V.upd[3 * u + 2] * 49, t / 7, t % 7);
    }
    for (int j = 0; j < V.nf; ++j) {
        const int b0 = V.col_ptr[j], b1 = V.col_ptr[j + 1];
        eg_fwd_diag(V.L + (size_t)b0 * 49, V.rhs + (size_t)j * 7);
        for (int b = b0 + 1; b < b1; ++b)
            for (int a = 0; a < 7; ++a) eg_fwd_row(V.L + (size_t)b * 49, V.rhs + (size_t)j * 7, V.rhs + (size_t)V.blk_row[b] * 7, a);
    }
    for (int j = V.nf - 1; j >= 0; --j) {
        double s[7];
        for (int a = 0; a < 7; ++a) s[a] = eg_back_gather(V, j, a);
        eg_back_diag(V.L + (size_t)V.col_ptr[j] * 49, s, V.rhs + (size_t)j * 7);
    }
    return true;
}

void trial(Host &H) {
    const EgView &V = H.V;
    bool failed = !factor_solve(V);
    double temp = 0.0, scale = 0.0;
    if (!failed) {
        for (int k = 0; k < V.nk; ++k) eg_vertex_step(V, k);
        for (int i = 0; i < V.nf; ++i) failed = failed || V.v_fail[i];
    }
    if (!failed) {
        for (int e = 0; e < V.ne; ++e) {
            eg_edge_trial(V, e);
            failed = failed || V.e_bad[e];
        }
    }
    if (!failed) {
        double c[64], s[64];
        for (int l = 0; l < 64; ++l) {
            c[l] = eg_edge_partial(V, V.chi_trial, 1, l);
            s[l] = eg_scale_partial(V, l);
        }
        temp = tree64(c);
        scale = tree64(s);
    }
    eg_judge(*V.st, failed, temp, scale);
}

}  // namespace

// S_init [nk][13] (R row-major, t, s), meas [ne][13]; ints [6]: iterations, trials, l_blocks, status, update triples, the plan's answer
// (EG_PLAN_*: not 0 = nothing else is written); doubles [3]: chi2_first, chi2_last, lambda; S_out, Swc_out [nk][13]; Tiw_out [nk][12]
extern "C" void essgraph_host(int nk, int fixed, int ne, const int *v0, const int *v1, const double *S_init, const double *meas, int iterations,
                              double lambda_init, int fix_scale, long long max_blocks, long long max_updates, int *ints, double *doubles, double *S_out,
                              double *Tiw_out, double *Swc_out) {
    Host H;
    EgView &V = H.V;
    std::memset(ints, 0, 6 * sizeof(int));
    std::memset(doubles, 0, 3 * sizeof(double));
    ints[5] = eg_plan(nk, fixed, ne, v0, v1, max_blocks, max_updates, H.P);
    if (ints[5]) return;
    const EgPlan &P = H.P;
    const int nf = P.nf;
    const size_t E = (size_t)(ne > 0 ? ne : 1), F = (size_t)(nf > 0 ? nf : 1);
    V.nk = nk; V.nf = nf; V.ne = ne; V.fixed = fixed; V.fix_scale = fix_scale; V.nob = P.nob; V.nb = P.nb; V.nu = P.nu;
    H.S.assign(2 * (size_t)nk * 13, 0.0);
    for (size_t q = 0; q < (size_t)nk * 13; ++q) H.S[q] = H.S[(size_t)nk * 13 + q] = S_init[q];
    H.pert.assign((size_t)nk * 14 * 13, 0.0); H.perr.assign(E * EG_NP * 7, 0.0); H.term.assign(E * EG_NT, 0.0); H.Hd.assign(F * 35, 0.0);
    H.Aoff.assign((size_t)(P.nob > 0 ? P.nob : 1) * 49, 0.0); H.L.assign((size_t)(P.nb > 0 ? P.nb : 1) * 49, 0.0); H.rhs.assign(F * 7, 0.0);
    H.chi_trial.assign(E, 0.0); H.e_bad.assign(E, 0); H.v_fail.assign(F, 0);
    V.v0 = v0; V.v1 = v1; V.meas = meas; V.S = H.S.data(); V.vertex_of = P.vertex_of.data(); V.sys_of = P.sys_of.data();
    V.ve_ptr = P.ve_ptr.data(); V.ve_edge = P.ve_edge.data(); V.ob_ptr = P.ob_ptr.data(); V.ob_edge = P.ob_edge.data();
    V.col_ptr = P.col_ptr.data(); V.blk_row = P.blk_row.data(); V.blk_col = P.blk_col.data(); V.blk_src = P.blk_src.data();
    V.upd_ptr = P.upd_ptr.data(); V.upd = P.upd.data();
    V.pert = H.pert.data(); V.perr = H.perr.data(); V.term = H.term.data(); V.Hd = H.Hd.data(); V.Aoff = H.Aoff.data(); V.L = H.L.data();
    V.rhs = H.rhs.data(); V.chi_trial = H.chi_trial.data(); V.e_bad = H.e_bad.data(); V.v_fail = H.v_fail.data(); V.solve_fail = &H.solve_fail;
    V.st = &H.st;
    EgStatus &S = H.st;
    S.ni = 2.0; S.max_it = iterations; S.next = EG_NEXT_ITERATION;
    if (nf == 0 || ne == 0 || iterations <= 0) {  // G8
        S.status = EG_EMPTY;
    } else {
        int next = EG_NEXT_ITERATION;
        while (next != EG_NEXT_DONE) {
            if (next == EG_NEXT_ITERATION) linearise(H, lambda_init);
            if (S.next == EG_NEXT_DONE) break;  // G5
            trial(H);
            next = S.next;
        }
    }
    ints[0] = S.iterations; ints[1] = S.trials; ints[2] = P.nb; ints[3] = S.status; ints[4] = P.nu;
    doubles[0] = S.chi2_first; doubles[1] = S.cur; doubles[2] = S.lam;
    for (int k = 0; k < nk; ++k)
        eg_recover(H.S.data() + ((size_t)S.buf * nk + k) * 13, S_out + (size_t)k * 13, Tiw_out + (size_t)k * 12, Swc_out + (size_t)k * 13);
}

// the point correction over plain arrays: pos [n][3] float (updated in place where a point moves), ok [n] (0: bad or unset), pair [n]
extern "C" void essgraph_host_correct(int n, float *pos, const uint8_t *ok, const int *pair, const double *S_from, const double *S_to, double *xyz_out,
                                      uint8_t *status) {
    for (int i = 0; i < n; ++i) {
        xyz_out[3 * (size_t)i] = xyz_out[3 * (size_t)i + 1] = xyz_out[3 * (size_t)i + 2] = 0.0;
        if (!ok[i]) {
            status[i] = EG_BAD_OR_UNSET;
        } else if (pair[i] < 0) {
            status[i] = EG_NO_PAIR;
        } else {
            const float P[3] = {pos[3 * (size_t)i], pos[3 * (size_t)i + 1], pos[3 * (size_t)i + 2]};
            double out[3];
            eg_correct(S_from + (size_t)pair[i] * 13, S_to + (size_t)pair[i] * 13, P, out);
            for (int c = 0; c < 3; ++c) {
                xyz_out[3 * (size_t)i + c] = out[c];
                pos[3 * (size_t)i + c] = (float)out[c];
            }
            status[i] = EG_MOVED;
        }
    }
}

#ifdef ESSGRAPH_HOST_MAIN
int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: essgraph_host scene.bin [max_blocks]\n");
        return 2;
    }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[6];
    double lambda_init;
    bool ok = std::fread(hdr, sizeof(int), 6, f) == 6 && std::fread(&lambda_init, sizeof(double), 1, f) == 1;
    const int nk = hdr[0], fixed = hdr[1], ne = hdr[2], np = hdr[5];
    ok = ok && nk >= 1 && nk <= 4096 && ne >= 0 && ne <= 65536 && fixed >= 0 && fixed < nk && np >= 0 && np <= 1 << 20;
    if (!ok) return 2;
    std::vector<double> S((size_t)nk * 13), meas((size_t)(ne > 0 ? ne : 1) * 13);
    std::vector<int> v0((size_t)(ne > 0 ? ne : 1)), v1((size_t)(ne > 0 ? ne : 1)), ref((size_t)(np > 0 ? np : 1));
    std::vector<float> pos((size_t)(np > 0 ? np : 1) * 3);
    std::vector<uint8_t> pok((size_t)(np > 0 ? np : 1)), pst((size_t)(np > 0 ? np : 1));
    ok = std::fread(S.data(), 8, (size_t)nk * 13, f) == (size_t)nk * 13 && std::fread(v0.data(), 4, (size_t)ne, f) == (size_t)ne &&
         std::fread(v1.data(), 4, (size_t)ne, f) == (size_t)ne && std::fread(meas.data(), 8, (size_t)ne * 13, f) == (size_t)ne * 13 &&
         std::fread(pos.data(), 4, (size_t)np * 3, f) == (size_t)np * 3 && std::fread(pok.data(), 1, (size_t)np, f) == (size_t)np &&
         std::fread(ref.data(), 4, (size_t)np, f) == (size_t)np;
    std::fclose(f);
    for (int e = 0; ok && e < ne; ++e) ok = v0[e] >= 0 && v0[e] < nk && v1[e] >= 0 && v1[e] < nk && v0[e] != v1[e];
    for (int i = 0; ok && i < np; ++i) ok = ref[i] >= -1 && ref[i] < nk;
    if (!ok) return 2;
    int ints[6];
    double d[3];
    std::vector<double> So((size_t)nk * 13), Tiw((size_t)nk * 12), Swc((size_t)nk * 13), xyz((size_t)(np > 0 ? np : 1) * 3);
    const long long max_blocks = argc > 2 ? std::atoll(argv[2]) : 131072;
    essgraph_host(nk, fixed, ne, v0.data(), v1.data(), S.data(), meas.data(), hdr[3], lambda_init, hdr[4], max_blocks, 2097152, ints, d, So.data(), Tiw.data(),
                  Swc.data());
    if (ints[5] == 0) essgraph_host_correct(np, pos.data(), pok.data(), ref.data(), S.data(), Swc.data(), xyz.data(), pst.data());
    int moved = 0;
    for (int i = 0; i < np; ++i) moved += ints[5] == 0 && pst[i] == EG_MOVED;
    std::printf("plan %d iterations %d trials %d l_blocks %d updates %d status %d chi2 %.17g %.17g lambda %.17g moved %d\n", ints[5], ints[0], ints[1], ints[2],
                ints[4], ints[3], d[0], d[1], d[2], moved);
    return 0;
}
#endif
