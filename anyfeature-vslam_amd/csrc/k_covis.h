// k_covis.h — what afv_covis.hip hands the kernels of k_covis.hip (kernel arguments; every pointer a device pointer)
#pragma once
#include "../../include/afv_covis.h"
#include "afv_runtime.h"

struct DevCovisQuery {
    const int *src;          // [n] the plane of the query's slot or the uploaded list
    int *dst;                // [n] the same entries, -1 where the id is not good (k_covis_filter)
    int n;
    int self;                // a slot query: its position in the keyframe list (votes[q][self] = 0); -1: an ids query
    int th, skip_bad;
};
struct DevCovisVotes {
    const int *mp;           // the table's planes [nsets][cap]
    int cap, nk, nq;
    const int *slots, *kf_n, *key_id;  // [nk]
    const uint8_t *kf_bad;   // [nk] or null
    const DevCovisQuery *queries;      // [nq]
    int *votes, *order;      // [nq][nk]
    int *n_order, *best, *n_nonzero;   // [nq]
};
struct DevCovisLocal {
    DevPointPlanes P;
    const int *mp;           // the table's planes
    int cap, nl;
    const int *local, *local_n;        // [nl]
    const int *frame_pts;    // [n_pts] or null
    int n_pts, max_out;
    unsigned *word;          // [P.cap] the store's first-occurrence words, 0xFFFFFFFF at rest
    int *pos;                // [P.cap] where a surviving id stands in ids_out (read only for ids whose word is not at rest)
    int *count;              // [nl] survivors per listed keyframe
    int *total;
    int *ids_out;            // [max_out]
    uint8_t *seen;           // [max_out], zeroed by the host side; null: not asked for
};
extern "C" void afv_launch_covis_votes(const DevPointPlanes *P, const DevCovisVotes *A, int max_n, hipStream_t stream);
extern "C" void afv_launch_covis_local(const DevCovisLocal *A, int max_n, hipStream_t stream);
