// covis_selftest — afv::CovisibilityVotes, afv::LocalPoints and afv::CovisibilityGraph (afv_adapter.hpp) as a plain C++ process, started by
// tests/test_gpu_covis_adapter.py.  Everything is an integer.
// Input (text): "nsets cap capacity th"; nsets lines "n id ..." (the plane of slot s); "nset id ..." the set ids; "nbad id ..." the bad ids;
// "nk" and nk lines "slot key_id bad"; "nq" and nq lines "kind position th skip_bad n id ..." (kind 0: a slot query, 1: ids);
// "nl slot ..." the local list; "npts id ..." the frame's points.
// Output: per query "Q best n_nonzero", "V votes ...", "O order ..."; "L ids ..." and "S seen ..." of LocalPoints; then the graph after
// UpdateConnectionsBatch of every listed slot with threshold th: per slot "G slot parent", "C ordered ...", "W weights ...", "N connected ..."
// (ascending keyId); essential_graph_dict(th): per keyframe not bad, ascending keyId, "E keyId parent" and "EC covisibles ..."; "B ..." and "D ..."
// = best_covisibles()(first slot) and connected(first slot); then UpdateLocalMap(frame points): "M valid ref", "K keyframes ...", "L ids ...", "S seen ...".
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "afv_adapter.hpp"

static void check(int rc, const char *what) {
    if (rc != AFV_OK) { std::fprintf(stderr, "%s: %s\n", what, afv_strerror(rc)); std::exit(1); }
}
static std::vector<int32_t> list(std::istream &in) {
    int n = 0;
    in >> n;
    std::vector<int32_t> v((size_t)n);
    for (int32_t &x : v) in >> x;
    return v;
}
template <class T>
static void line(const char *tag, const std::vector<T> &v) {
    std::printf("%s", tag);
    for (const T &x : v) std::printf(" %d", (int)x);
    std::printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    int nsets = 0, cap = 0, capacity = 0, th = 15;
    in >> nsets >> cap >> capacity >> th;
    afv_orb_params prm;
    afv_default_orb_params(&prm);
    afv_ctx *ctx = nullptr;
    check(afv_create(0, &prm, &ctx), "afv_create");
    afv_table *table = nullptr;
    check(afv_table_create(ctx, nsets, cap, &table), "afv_table_create");
    for (int s = 0; s < nsets; ++s) {
        const std::vector<int32_t> plane = list(in);
        const std::vector<uint8_t> rows(plane.size() * 32 + 1, 0);
        check(afv_table_set(table, s, rows.data(), nullptr, (int)plane.size()), "afv_table_set");
        check(afv_table_set_map_points(table, s, plane.data()), "afv_table_set_map_points");
    }
    {
        afv::DeviceMapPoints points(ctx, capacity);
        const std::vector<int32_t> set_ids = list(in), bad_ids = list(in);
        const std::vector<float> xyz(set_ids.size() * 3 + 1, 0.0f);
        const std::vector<uint8_t> ones(bad_ids.size() + 1, 1);
        if (!set_ids.empty()) points.SetWorldPos(set_ids, xyz.data());
        if (!bad_ids.empty()) points.SetFlags(bad_ids, ones.data(), nullptr);
        int nk = 0, nq = 0;
        in >> nk;
        std::vector<int32_t> slots((size_t)nk), keys((size_t)nk);
        std::vector<uint8_t> bad((size_t)nk);
        for (int k = 0; k < nk; ++k) {
            int b = 0;
            in >> slots[(size_t)k] >> keys[(size_t)k] >> b;
            bad[(size_t)k] = (uint8_t)b;
        }
        in >> nq;
        std::vector<std::vector<int32_t>> lists((size_t)nq);
        std::vector<afv::CovisQuery> qs((size_t)nq);
        for (int q = 0; q < nq; ++q) {
            int kind = 0, skip = 0;
            in >> kind >> qs[(size_t)q].position >> qs[(size_t)q].th >> skip;
            qs[(size_t)q].skip_bad = skip != 0;
            lists[(size_t)q] = list(in);
            if (kind == 1) qs[(size_t)q].ids = &lists[(size_t)q];
        }
        const std::vector<int32_t> local = list(in), frame_pts = list(in);
        if (nq > 0) {
            const afv::CovisAnswer A = afv::CovisibilityVotes(ctx, table, points, slots, keys, &bad, qs);
            for (int q = 0; q < nq; ++q) {
                std::printf("Q %d %d\n", A.best[(size_t)q], A.n_nonzero[(size_t)q]);
                line("V", A.votes[(size_t)q]);
                line("O", A.order[(size_t)q]);
            }
        }
        const afv::LocalPointsAnswer L = afv::LocalPoints(ctx, table, cap, points, local, &frame_pts);
        line("L", L.ids);
        line("S", L.seen);
        afv::CovisibilityGraph g(ctx, table, cap, points);
        g.th = th;
        for (int k = 0; k < nk; ++k) {
            g.add_keyframe(slots[(size_t)k], keys[(size_t)k]);
            if (bad[(size_t)k]) g.set_bad(slots[(size_t)k]);
        }
        g.UpdateConnectionsBatch(slots);
        for (int32_t s : slots) {
            std::printf("G %d %d\n", s, g.GetParent(s));
            line("C", g.GetVectorCovisibleKeyFrames(s));
            line("W", g.GetNode(s).ordered_w);
            line("N", g.GetConnectedKeyFrames(s));
        }
        const afv::CovisibilityGraph::EssentialGraphPieces P = g.essential_graph_dict(th);
        for (const auto &e : P.parent) {
            std::printf("E %d %d\n", e.first, e.second);
            line("EC", P.covisibles.at(e.first));
        }
        if (nk > 0) {
            line("B", g.best_covisibles()(slots[0]));
            line("D", g.connected(slots[0]));
        }
        const afv::CovisibilityGraph::LocalMap M = g.UpdateLocalMap(frame_pts, 80, 10);
        std::printf("M %d %d\n", M.valid ? 1 : 0, M.ref);
        line("K", M.keyframes);
        line("L", M.ids);
        line("S", M.seen);
    }
    afv_table_destroy(table);
    afv_destroy(ctx);
    return 0;
}
