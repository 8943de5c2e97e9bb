/* afv_covis.h — C-ABI of the covisibility count and the local map, same library as afv_hip.h (libafv_hip.so).
 *
 * Reference: KeyFrame::UpdateConnections (KeyFrame.cc:329-418), Tracking::UpdateLocalKeyFrames / UpdateLocalPoints (Tracking.cc:1040-1104)
 * and the skip of Tracking::SearchLocalPoints (Tracking.cc:1003-1005).  The reference walks MapPoint::GetObservations(); here the question
 * "does keyframe k observe point p" is answered from what is already resident: slot s observes id p when p occurs in the slot's
 * mvpMapPoints plane (afv_table_set_map_points), positions [0, n_s).  No observation list is uploaded.
 *
 * A GOOD ID (V1): 0 <= id < capacity of the store, set, and not bad.  Everything else (-1, an id outside the store, a never-set id, a bad
 * id) is skipped, in a query and in a plane alike: the reference's `pt && !pt->isBad()`.
 *
 * New symbols and records only: AFV_ABI_VERSION stays 6. */
#ifndef AFV_COVIS_H
#define AFV_COVIS_H
#include <stddef.h>
#include <stdint.h>

#include "afv_hip.h" /* afv_table, afv_points, error codes */
#ifdef __cplusplus
extern "C" {
#endif

#define AFV_COVIS_MAX_IDS 65536   /* entries of one ids query */
#define AFV_COVIS_MAX_QUERIES 64  /* queries that share one pass over the planes */
#define AFV_COVIS_MAX_LOCAL 256   /* keyframes of one local map */
#define AFV_COVIS_MAX_KF 4096     /* listed keyframes of one votes call */
#define AFV_COVIS_MAX_CAP 4096    /* features per slot of a table these calls take (the id set of a plane lives in the LDS): the largest
                                     table afv_table_create makes.  A larger one would be AFV_EUNSUPPORTED */

enum { AFV_COVIS_QUERY_SLOT = 0, AFV_COVIS_QUERY_IDS = 1 };

/* One query of afv_table_covis_votes.  struct_size first, as in every versioned record of afv_hip.h.
 *   AFV_COVIS_QUERY_SLOT: `position` names an entry of the call's keyframe list; the query is that slot's plane and the keyframe does not
 *                         vote for itself (obs.first == keyId).  ids / n are not read.
 *   AFV_COVIS_QUERY_IDS:  `ids[n]`, a host list of point ids in [-1, capacity); nothing is excluded (the frame's pts).
 * th: the connection threshold (15 in UpdateConnections, 1 for the local map).  skip_bad: keyframes whose kf_bad is set keep their votes but
 * stand in neither order nor best (Tracking.cc:1087); UpdateConnections itself runs with 0. */
typedef struct {
    uint32_t struct_size;
    int32_t kind;
    int32_t position;
    int32_t n;
    const int32_t *ids;
    int32_t th;
    int32_t skip_bad;
} afv_covis_query;

/* votes[q][k] = #{ i : Q_q[i] good and Q_q[i] in plane(slots[k]) } for the nk listed keyframes (slots[nk] distinct table slots with a
 * plane, key_id[nk] distinct, any order) and nq queries.  An id twice in Q counts twice; an id twice in a plane counts once.
 * Per query, row-major [nq][nk]:
 *   order[q][0 .. n_order[q])  the positions with votes >= th (and > 0), votes descending, ties by key_id DESCENDING; -1 behind them.
 *                              Nobody at th and best >= 0: {best} alone.
 *   best[q]                    the position of the highest vote, ties to the LOWEST key_id; -1 when every vote is 0
 *   n_nonzero[q]               positions with a vote
 * votes and order may be NULL.  One upload, the launches on the context's stream, one wait.
 * Refused before any launch, outputs untouched (AFV_EINVAL unless noted): a NULL required argument, nk outside 1 .. AFV_COVIS_MAX_KF, nq
 * outside 1 .. AFV_COVIS_MAX_QUERIES, a slot out of range, listed twice or without a plane, a duplicate key_id, a position outside [0, nk),
 * an unknown kind or struct_size, n outside 0 .. AFV_COVIS_MAX_IDS, an id outside [-1, capacity), skip_bad without kf_bad, store and table
 * on different contexts; a table of more than AFV_COVIS_MAX_CAP features per slot AFV_EUNSUPPORTED. */
int afv_table_covis_votes(afv_table *t, afv_points *points, const int32_t *slots, const int32_t *key_id, const uint8_t *kf_bad, int nk,
                          const afv_covis_query *queries, int nq, int32_t *votes, int32_t *order, int32_t *n_order, int32_t *best,
                          int32_t *n_nonzero);

/* Tracking::UpdateLocalPoints over local[nl], the table slots in the order of localKeyframes: the good ids of their planes, slots in list
 * order, features in ascending index, every id at its first occurrence only.  *n_out = the total.  frame_pts[n_pts] (may be NULL) with
 * seen_out: seen_out[j] = 1 where local point j is a good id of that list (the points SearchLocalPoints skips), else 0.
 * A total beyond max_out answers AFV_ECAPACITY and writes nothing.  nl == 0: *n_out = 0.  The answer does not depend on earlier calls: the
 * store's first-occurrence words are back at rest when the call returns, AFV_ECAPACITY included.
 * Refused before any launch, outputs and store untouched (AFV_EINVAL unless noted): a NULL required argument, nl outside 0 ..
 * AFV_COVIS_MAX_LOCAL, max_out < 0, a slot out of range, listed twice or without a plane, n_pts outside 0 .. AFV_COVIS_MAX_IDS, an id of
 * frame_pts outside [-1, capacity), store and table on different contexts; a table of more than AFV_COVIS_MAX_CAP features per slot
 * AFV_EUNSUPPORTED.  seen_out without frame_pts reads 0 everywhere. */
int afv_table_local_points(afv_table *t, afv_points *points, const int32_t *local, int nl, const int32_t *frame_pts, int n_pts, int max_out,
                           int32_t *ids_out, uint8_t *seen_out, int32_t *n_out);

#ifdef __cplusplus
}
#endif
#endif
