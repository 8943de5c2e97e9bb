// afv_gba_plan.h — what the host derives from the edge list of a global bundle adjustment while it checks the arguments (L7' of
// tests/_gba_ref.py): the structural blocks of the reduced camera system (block (i, j) exists when some listed point has an edge to both
// free keyframes - from the edge list as given, before the gather drops points and before any check removes edges, so the pattern is a
// superset and a block that became empty holds exact zeros), the symbolic factorisation in the order of the free-keyframe list (the
// column structure of L) and which blocks of L a trial evaluates.  No per-column update triples are kept: the kernel finds an update's
// target by a binary search in the target column's rows.  Host code only; shared by afv_lba.hip and tools/lba_host.cpp.
#pragma once

#include <algorithm>
#include <cstdint>
#include <iterator>
#include <vector>

struct GbPlan {
    int nf = 0, nb = 0, ns = 0;   // free keyframes, blocks of L, structural blocks among them (diagonal blocks included)
    std::vector<int> col_ptr, blk_row, blk_col;
    std::vector<uint8_t> blk_kind;
};

#define GB_PLAN_OK 0
#define GB_PLAN_BLOCKS 1   // the fill exceeds max_blocks

// pt_ptr [np + 1], e_kf [ne]: the edges by point; a keyframe at a position >= nf is fixed.  The caller has checked the ranges and that no
// keyframe observes a point twice.  A point seen by d free keyframes costs d (d - 1) / 2 visits of a bit matrix of nf x nf bits (2 MiB
// at 4096 keyframes).
static inline int gb_plan(int nf, int np, const int *pt_ptr, const int32_t *e_kf, long long max_blocks, GbPlan &P) {
    P.nf = nf;
    const size_t words = ((size_t)nf + 63) / 64;
    std::vector<uint64_t> bits((size_t)nf * words, 0);   // row lo, bit hi > lo
    std::vector<int> seen;
    for (int p = 0; p < np; ++p) {
        seen.clear();
        for (int e = pt_ptr[p]; e < pt_ptr[p + 1]; ++e)
            if (e_kf[e] < nf) seen.push_back(e_kf[e]);
        for (size_t x = 0; x < seen.size(); ++x)
            for (size_t y = x + 1; y < seen.size(); ++y) {
                const int lo = std::min(seen[x], seen[y]), hi = std::max(seen[x], seen[y]);
                bits[(size_t)lo * words + (size_t)(hi >> 6)] |= 1ull << (hi & 63);
            }
    }
    auto structural = [&](int lo, int hi) { return (bits[(size_t)lo * words + (size_t)(hi >> 6)] >> (hi & 63)) & 1ull; };
    std::vector<std::vector<int>> rows((size_t)nf);      // struct(j), ascending
    for (int j = 0; j < nf; ++j)
        for (size_t w = 0; w < words; ++w) {
            uint64_t v = bits[(size_t)j * words + w];
            while (v) {
                rows[(size_t)j].push_back((int)(w * 64) + __builtin_ctzll(v));
                v &= v - 1;
            }
        }
    // the symbolic factorisation: struct(parent) receives struct(j) without the parent
    long long nb = 0;
    for (int j = 0; j < nf; ++j) {
        const std::vector<int> &r = rows[(size_t)j];
        nb += 1 + (long long)r.size();
        if (nb > max_blocks) return GB_PLAN_BLOCKS;
        if (r.size() > 1) {
            std::vector<int> &p = rows[(size_t)r[0]], merged;
            merged.reserve(p.size() + r.size());
            std::set_union(p.begin(), p.end(), r.begin() + 1, r.end(), std::back_inserter(merged));
            p.swap(merged);
        }
    }
    P.nb = (int)nb;
    P.ns = 0;
    P.col_ptr.assign((size_t)nf + 1, 0);
    P.blk_row.assign((size_t)std::max<long long>(nb, 1), 0);
    P.blk_col.assign((size_t)std::max<long long>(nb, 1), 0);
    P.blk_kind.assign((size_t)std::max<long long>(nb, 1), 0);
    for (int j = 0, b = 0; j < nf; ++j) {
        P.col_ptr[(size_t)j] = b;
        P.blk_row[(size_t)b] = j;
        P.blk_col[(size_t)b] = j;
        P.blk_kind[(size_t)b++] = 1;
        ++P.ns;
        for (int i : rows[(size_t)j]) {
            P.blk_row[(size_t)b] = i;
            P.blk_col[(size_t)b] = j;
            const uint8_t k = structural(j, i) ? 1 : 0;
            P.ns += k;
            P.blk_kind[(size_t)b++] = k;
        }
        P.col_ptr[(size_t)j + 1] = b;
    }
    return GB_PLAN_OK;
}
