// covis_host.cpp — the covisibility count and the local map (include/afv_covis.h) as scalar host code over flat arrays: the route
// tools/time_covis.py times the device against, and a second answer to every scene of tests/_covis_scenes.py (tests/test_covis_ref_cpu.py).
// Not the reference's maps: the planes as one int array, the store as a flag byte per id, and stamp arrays instead of std::set / std::map -
// a word per id that holds the token of the pass that last touched it, so nothing is cleared between passes.
//   g++ -O3 -std=c++17 -shared -fPIC tools/covis_host.cpp -o tools/libcovis_host.so
#include <algorithm>
#include <cstdint>
#include <vector>

namespace {
struct Host {
    int capacity;
    std::vector<uint32_t> q_stamp, k_stamp;  // token of the query / keyframe pass that last touched the id
    std::vector<int32_t> mult;                // how often the id stands in the query (valid where q_stamp holds the query's token)
    uint32_t token = 0;
};
inline bool good(const uint8_t *flags, int capacity, int id) { return id >= 0 && id < capacity && (flags[id] & 1) && !(flags[id] & 2); }
}  // namespace

extern "C" {

void *covis_host_create(int capacity) {
    Host *h = new Host();
    h->capacity = capacity;
    h->q_stamp.assign((size_t)capacity, 0);
    h->k_stamp.assign((size_t)capacity, 0);
    h->mult.assign((size_t)capacity, 0);
    return h;
}
void covis_host_destroy(void *p) { delete static_cast<Host *>(p); }

// planes [nsets][cap], n [nsets]; flags [capacity]: bit 0 set, bit 1 bad.  Queries: kind 0 = slot (q_pos), 1 = ids q_ids[q_ptr[q] .. q_ptr[q + 1]).
// votes / order [nq][nk], n_order / best / n_nonzero [nq]
void covis_host_votes(void *hp, const int32_t *planes, const int32_t *n, int cap, const uint8_t *flags, const int32_t *slots, const int32_t *key_id,
                      const uint8_t *kf_bad, int nk, int nq, const int32_t *q_kind, const int32_t *q_pos, const int32_t *q_ptr, const int32_t *q_ids,
                      const int32_t *q_th, const int32_t *q_skip, int32_t *votes, int32_t *order, int32_t *n_order, int32_t *best, int32_t *n_nonzero) {
    Host &H = *static_cast<Host *>(hp);
    std::vector<int> members;
    for (int q = 0; q < nq; ++q) {
        const int32_t *Q;
        int nQ, self = -1;
        if (q_kind[q] == 0) {
            self = q_pos[q];
            Q = planes + (size_t)slots[self] * cap;
            nQ = n[slots[self]];
        } else {
            Q = q_ids + q_ptr[q];
            nQ = q_ptr[q + 1] - q_ptr[q];
        }
        const uint32_t qt = ++H.token;
        for (int i = 0; i < nQ; ++i) {
            const int id = Q[i];
            if (!good(flags, H.capacity, id)) continue;
            if (H.q_stamp[(size_t)id] != qt) { H.q_stamp[(size_t)id] = qt; H.mult[(size_t)id] = 0; }
            ++H.mult[(size_t)id];  // twice in Q: counted twice
        }
        int32_t *row = votes + (size_t)q * nk, *ord = order + (size_t)q * nk;
        int nz = 0, b = -1, nmax = 0;
        members.clear();
        for (int k = 0; k < nk; ++k) {
            int v = 0;
            if (k != self) {
                const int32_t *P = planes + (size_t)slots[k] * cap;
                const int nP = n[slots[k]];
                const uint32_t kt = ++H.token;
                for (int i = 0; i < nP; ++i) {
                    const int id = P[i];
                    if (id < 0 || id >= H.capacity || H.q_stamp[(size_t)id] != qt || H.k_stamp[(size_t)id] == kt) continue;
                    H.k_stamp[(size_t)id] = kt;  // twice in the plane: counted once
                    v += H.mult[(size_t)id];
                }
            }
            row[k] = v;
            ord[k] = -1;
            nz += v > 0;
            if (v <= 0 || (q_skip[q] && kf_bad[k])) continue;
            if (v > nmax || (v == nmax && key_id[k] < key_id[b])) { nmax = v; b = k; }  // ties: the lowest keyId
            if (v >= q_th[q]) members.push_back(k);
        }
        if (members.empty() && b >= 0) members.push_back(b);
        std::sort(members.begin(), members.end(), [&](int a, int c) { return row[a] != row[c] ? row[a] > row[c] : key_id[a] > key_id[c]; });
        std::copy(members.begin(), members.end(), ord);
        n_order[q] = (int)members.size();
        best[q] = b;
        n_nonzero[q] = nz;
    }
}

// the good ids of the planes of local[nl] at their first occurrence; seen[j] = 1 where ids_out[j] is a good id of frame_pts.  Returns the total
int covis_host_local(void *hp, const int32_t *planes, const int32_t *n, int cap, const uint8_t *flags, const int32_t *local, int nl,
                     const int32_t *frame_pts, int n_pts, int32_t *ids_out, uint8_t *seen) {
    Host &H = *static_cast<Host *>(hp);
    const uint32_t ft = ++H.token;
    for (int i = 0; i < n_pts; ++i)
        if (good(flags, H.capacity, frame_pts[i])) H.q_stamp[(size_t)frame_pts[i]] = ft;
    const uint32_t lt = ++H.token;
    int total = 0;
    for (int l = 0; l < nl; ++l) {
        const int32_t *P = planes + (size_t)local[l] * cap;
        const int nP = n[local[l]];
        for (int i = 0; i < nP; ++i) {
            const int id = P[i];
            if (!good(flags, H.capacity, id) || H.k_stamp[(size_t)id] == lt) continue;
            H.k_stamp[(size_t)id] = lt;
            if (seen) seen[total] = H.q_stamp[(size_t)id] == ft;
            ids_out[total++] = id;
        }
    }
    return total;
}

}  // extern "C"
