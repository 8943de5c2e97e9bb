// afv_essgraph_plan.h — what the host derives from the edge list of an essential graph while it checks the arguments (G1, G6 of
// tests/_essgraph_ref.py): the system positions, the by-vertex order of the edges (a counting sort, as the bundle adjustment's), the
// off-diagonal blocks of H with their edges, the symbolic factorisation in the order of the keyframe list (the column structure of L)
// and, per column, the update triples.  Host code only; shared by afv_essgraph.hip and tools/essgraph_host.cpp.
#pragma once

#include <algorithm>
#include <cstdint>
#include <iterator>
#include <vector>

struct EgPlan {
    int nf = 0, nob = 0, nb = 0, nu = 0;
    std::vector<int> vertex_of, sys_of, ve_ptr, ve_edge, ob_ptr, ob_edge, col_ptr, blk_row, blk_col, blk_src, upd_ptr, upd;
};

#define EG_PLAN_OK 0
#define EG_PLAN_BLOCKS 1   // the fill exceeds max_blocks
#define EG_PLAN_UPDATES 2  // the update triples exceed max_updates

// the caller has checked: 0 <= fixed < nk, 0 <= v0, v1 < nk, v0 != v1
static inline int eg_plan(int nk, int fixed, int ne, const int32_t *v0, const int32_t *v1, long long max_blocks, long long max_updates, EgPlan &P) {
    const int nf = nk - 1;
    P.nf = nf;
    P.sys_of.assign((size_t)nk, -1);
    P.vertex_of.assign((size_t)std::max(nf, 1), 0);
    for (int k = 0, i = 0; k < nk; ++k)
        if (k != fixed) {
            P.sys_of[(size_t)k] = i;
            P.vertex_of[(size_t)i++] = k;
        }
    // the edges of every free vertex in list order
    P.ve_ptr.assign((size_t)nf + 1, 0);
    for (int e = 0; e < ne; ++e) {
        const int a = P.sys_of[(size_t)v0[e]], b = P.sys_of[(size_t)v1[e]];
        if (a >= 0) ++P.ve_ptr[(size_t)a + 1];
        if (b >= 0) ++P.ve_ptr[(size_t)b + 1];
    }
    for (int i = 0; i < nf; ++i) P.ve_ptr[(size_t)i + 1] += P.ve_ptr[(size_t)i];
    P.ve_edge.assign((size_t)P.ve_ptr[(size_t)nf] + 1, 0);
    {
        std::vector<int> at(P.ve_ptr.begin(), P.ve_ptr.end());
        for (int e = 0; e < ne; ++e) {
            const int a = P.sys_of[(size_t)v0[e]], b = P.sys_of[(size_t)v1[e]];
            if (a >= 0) P.ve_edge[(size_t)at[(size_t)a]++] = 2 * e;
            if (b >= 0) P.ve_edge[(size_t)at[(size_t)b]++] = 2 * e + 1;
        }
    }
    // the off-diagonal blocks of H: per column (the earlier vertex) the rows with their edges; a stable sort keeps the list order
    struct Ref { int lo, hi, code; };
    std::vector<Ref> refs;
    for (int e = 0; e < ne; ++e) {
        const int a = P.sys_of[(size_t)v0[e]], b = P.sys_of[(size_t)v1[e]];
        if (a >= 0 && b >= 0) refs.push_back(Ref{std::min(a, b), std::max(a, b), 2 * e + (a < b ? 1 : 0)});
    }
    std::stable_sort(refs.begin(), refs.end(), [](const Ref &x, const Ref &y) { return x.lo != y.lo ? x.lo < y.lo : x.hi < y.hi; });
    std::vector<std::vector<int>> rows((size_t)nf);   // struct(j), ascending
    std::vector<int> ob_lo, ob_hi;
    P.ob_ptr.assign(1, 0);
    P.ob_edge.clear();
    for (size_t q = 0; q < refs.size(); ++q) {
        if (q == 0 || refs[q].lo != refs[q - 1].lo || refs[q].hi != refs[q - 1].hi) {
            if (q) P.ob_ptr.push_back((int)P.ob_edge.size());
            ob_lo.push_back(refs[q].lo);
            ob_hi.push_back(refs[q].hi);
            rows[(size_t)refs[q].lo].push_back(refs[q].hi);
        }
        P.ob_edge.push_back(refs[q].code);
    }
    P.nob = (int)ob_lo.size();
    P.ob_ptr.push_back((int)P.ob_edge.size());
    P.ob_edge.push_back(0);
    // the symbolic factorisation: struct(parent) receives struct(j) without the parent
    long long nb = 0, nu = 0;
    for (int j = 0; j < nf; ++j) {
        const std::vector<int> &r = rows[(size_t)j];
        const long long m = (long long)r.size();
        nb += 1 + m;
        nu += m * (m + 1) / 2;
        if (nb > max_blocks) return EG_PLAN_BLOCKS;
        if (nu > max_updates) return EG_PLAN_UPDATES;
        if (m > 1) {
            std::vector<int> &p = rows[(size_t)r[0]], merged;
            merged.reserve(p.size() + r.size());
            std::set_union(p.begin(), p.end(), r.begin() + 1, r.end(), std::back_inserter(merged));
            p.swap(merged);
        }
    }
    P.nb = (int)nb;
    P.nu = (int)nu;
    P.col_ptr.assign((size_t)nf + 1, 0);
    P.blk_row.assign((size_t)std::max<long long>(nb, 1), 0);
    P.blk_col.assign((size_t)std::max<long long>(nb, 1), 0);
    P.blk_src.assign((size_t)std::max<long long>(nb, 1), -1);
    for (int j = 0, b = 0; j < nf; ++j) {
        P.col_ptr[(size_t)j] = b;
        P.blk_row[(size_t)b] = j;
        P.blk_col[(size_t)b++] = j;
        for (int i : rows[(size_t)j]) {
            P.blk_row[(size_t)b] = i;
            P.blk_col[(size_t)b++] = j;
        }
        P.col_ptr[(size_t)j + 1] = b;
    }
    auto block_of = [&](int i, int k) {  // the block (row i, column k) of L
        if (i == k) return P.col_ptr[(size_t)k];
        const std::vector<int> &r = rows[(size_t)k];
        return P.col_ptr[(size_t)k] + 1 + (int)(std::lower_bound(r.begin(), r.end(), i) - r.begin());
    };
    for (int q = 0; q < P.nob; ++q) P.blk_src[(size_t)block_of(ob_hi[(size_t)q], ob_lo[(size_t)q])] = q;
    P.upd_ptr.assign((size_t)nf + 1, 0);
    P.upd.assign(3 * (size_t)std::max<long long>(nu, 1), 0);
    size_t u = 0;
    for (int j = 0; j < nf; ++j) {
        const std::vector<int> &r = rows[(size_t)j];
        const int b0 = P.col_ptr[(size_t)j] + 1;
        for (size_t qi = 0; qi < r.size(); ++qi)
            for (size_t qk = 0; qk <= qi; ++qk) {
                P.upd[3 * u] = b0 + (int)qi;
                P.upd[3 * u + 1] = b0 + (int)qk;
                P.upd[3 * u + 2] = block_of(r[qi], r[qk]);
                ++u;
            }
        P.upd_ptr[(size_t)j + 1] = (int)u;
    }
    return EG_PLAN_OK;
}
