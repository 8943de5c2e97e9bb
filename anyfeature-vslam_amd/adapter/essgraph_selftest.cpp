// essgraph_selftest — afv::OptimizeEssentialGraph and afv::CorrectPointsSim3 (afv_adapter.hpp) as a plain C++ process, started by
// tests/test_gpu_essgraph_adapter.py.  Input (binary, the scene file of tools/essgraph_host.cpp): int32 nk, fixed, ne, iterations,
// fix_scale, np; double lambda_init; S_init [nk][13]; v0 [ne]; v1 [ne]; meas [ne][13]; pos [np][3] float; ok [np] bytes; ref [np] int32.
// Point i has id i in a store of np + 3 points; a point that is not ok is bad.  Output (binary): int32 iterations, trials, l_blocks, status;
// double chi2_first, chi2_last, lambda; CorrectedSiw [nk][13]; Tiw [nk][12]; xyz [np][3]; the store's positions [np][3] float after the
// call; point_status [np]; then status [np] and the positions [np][3] of a second store after afv::CorrectPointsSim3 with the same pairs.
#include <cstdio>
#include <cstdlib>

#include "afv_adapter.hpp"

static void check(int rc, const char *what) {
    if (rc != AFV_OK) { std::fprintf(stderr, "%s: %s\n", what, afv_strerror(rc)); std::exit(1); }
}

template <class T>
static bool rd(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n > 0 ? n : 1);
    return std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[6];
    double lambda_init = 0.0;
    if (std::fread(hdr, 4, 6, f) != 6 || std::fread(&lambda_init, 8, 1, f) != 1) return 2;
    const int nk = hdr[0], fixed = hdr[1], ne = hdr[2], np = hdr[5];
    if (nk < 1 || nk > AFV_ESS_MAX_KF || ne < 0 || ne > AFV_ESS_MAX_EDGES || np < 0 || np > 100000) return 2;
    std::vector<afv_sim3d> S, meas;
    std::vector<int32_t> v0, v1, ref;
    std::vector<float> pos;
    std::vector<uint8_t> ok;
    if (!rd(f, S, nk) || !rd(f, v0, ne) || !rd(f, v1, ne) || !rd(f, meas, ne) || !rd(f, pos, (size_t)np * 3) || !rd(f, ok, np) || !rd(f, ref, np)) return 2;
    std::fclose(f);
    S.resize(nk); ref.resize(np);
    afv_orb_params prm;
    afv_default_orb_params(&prm);
    afv_ctx *ctx = nullptr;
    check(afv_create(0, &prm, &ctx), "afv_create");
    std::vector<afv::EssentialGraphEdge> edges((size_t)ne);
    for (int e = 0; e < ne; ++e) edges[e] = afv::EssentialGraphEdge{v0[e], v1[e], meas[e]};
    std::vector<int32_t> ids((size_t)np);
    std::vector<uint8_t> bad((size_t)(np > 0 ? np : 1));
    for (int i = 0; i < np; ++i) { ids[i] = i; bad[i] = ok[i] ? 0 : 1; }
    int rc = 0;
    {
        afv::DeviceMapPoints one(ctx, np + 3), two(ctx, np + 3);
        if (np > 0) {
            one.SetWorldPos(ids, pos.data()); one.SetFlags(ids, bad.data(), nullptr);
            two.SetWorldPos(ids, pos.data()); two.SetFlags(ids, bad.data(), nullptr);
        }
        const afv::EssentialGraphAnswer A = afv::OptimizeEssentialGraph(ctx, &one, S, fixed, edges, hdr[4] != 0, ids, ref, hdr[3], lambda_init);
        std::vector<afv_sim3d> Swc((size_t)nk);
        for (int k = 0; k < nk; ++k) {  // Sim3::inverse of the answer, for the second store: the same operators as the library's
            const afv_sim3d &E = A.CorrectedSiw[k];
            afv_sim3d &I = Swc[k];
            const double m = -1.0 / E.s, t0 = E.t[0] * m, t1 = E.t[1] * m, t2 = E.t[2] * m;
            for (int i = 0; i < 3; ++i) {
                for (int j = 0; j < 3; ++j) I.R[3 * i + j] = E.R[3 * j + i];
                I.t[i] = E.R[i] * t0 + (E.R[3 + i] * t1 + E.R[6 + i] * t2);
            }
            I.s = 1.0 / E.s;
        }
        const std::vector<uint8_t> st2 = afv::CorrectPointsSim3(ctx, two, ids, ref, S, Swc);
        std::vector<float> after((size_t)(np > 0 ? np : 1) * 3), after2((size_t)(np > 0 ? np : 1) * 3);
        if (np > 0) {
            check(afv_points_get(one.handle(), ids.data(), np, after.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "afv_points_get");
            check(afv_points_get(two.handle(), ids.data(), np, after2.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "afv_points_get");
        }
        FILE *o = std::fopen(argv[2], "wb");
        if (!o) return 2;
        const int32_t ints[4] = {A.trace.iterations, A.trace.trials, A.trace.l_blocks, A.trace.status};
        const double d[3] = {A.trace.chi2_first, A.trace.chi2_last, A.trace.lambda};
        std::fwrite(ints, 4, 4, o); std::fwrite(d, 8, 3, o);
        std::fwrite(A.CorrectedSiw.data(), sizeof(afv_sim3d), (size_t)nk, o); std::fwrite(A.Tiw.data(), 8, (size_t)nk * 12, o);
        std::fwrite(A.xyz.data(), 8, (size_t)np * 3, o); std::fwrite(after.data(), 4, (size_t)np * 3, o); std::fwrite(A.point_status.data(), 1, (size_t)np, o);
        std::fwrite(st2.data(), 1, (size_t)np, o); std::fwrite(after2.data(), 4, (size_t)np * 3, o);
        rc = std::fclose(o) == 0 ? 0 : 1;
    }
    afv_destroy(ctx);
    return rc;
}
