// afv_voctrain.h — records and launcher prototypes shared by k_voctrain.hip (the kernels) and afv_voctrain.hip (the host runtime of
// afv_vocab_train).  Not part of the public interface.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define VT_THREADS 256
#define VT_TILE 4096  // rows of one node a workgroup takes: a node of more rows spans several tiles ("multi-tile" node)
#define VT_DRAW_STEP 0xD1342543DE82EF95ull

struct VtTile {
    int node, start, len;  // node index within the level, first row position, rows
};
struct VtNode {
    int start, len;      // the node's contiguous, order-preserving segment of the row array
    int tile0, ntiles;   // its tiles
    int slot, pad;       // multi-tile nodes: index into the global count tables; -1: the node is one tile
    unsigned long long key;  // generator key of the node (a function of the seed and the path from the root)
};

// everything a level's kernels touch; the arrays are per level except rows / assign / mindist (per row position)
struct VtArgs {
    const VtTile *tiles;
    const VtNode *nodes;
    const int *multi;      // [nmulti] node indices of the multi-tile nodes
    int ntiles, nnodes, nmulti, k, words;
    const uint32_t *rows;  // [n][words] in the level's order
    uint32_t *rows_out;    // the next level's order (stable partition by cluster)
    uint8_t *assign;       // [n] cluster of the row at a position
    int32_t *mindist;      // [n] seeding: distance to the nearest centre so far
    uint32_t *centres;     // [nnodes][k][words]
    int *ncent, *done, *seeded, *changed;  // [nnodes]
    int *sizes;            // [nnodes][k] cluster sizes of the last association
    uint32_t *gcnt;        // [nmulti][bits][k] per-(cluster, bit) counts of the multi-tile nodes
    int *gsize;            // [nmulti][k]
    long long *tile_sum;   // [ntiles]
    int *tile_hist, *tile_off;  // [ntiles][k]
    int *status;           // [0] nodes that go on to another round, [1] some node stopped at max_iters unconverged
    int round, max_iters, draw;
};

extern "C" int afv_voctrain_prepare(void);
extern "C" size_t afv_voctrain_assoc_lds(int k, int words);
extern "C" void afv_launch_vt_pad(const uint8_t *src, size_t pitch, int desc_bytes, long long n, int words, uint32_t *dst, hipStream_t stream);
extern "C" void afv_launch_vt_seed_first(const VtArgs *a, hipStream_t stream);
extern "C" void afv_launch_vt_seed_draw(const VtArgs *a, hipStream_t stream);  // min-distance update + segmented sum + pick, draw a->draw
extern "C" void afv_launch_vt_round(const VtArgs *a, hipStream_t stream);      // association + counts (+ majority), round a->round
extern "C" void afv_launch_vt_partition(const VtArgs *a, hipStream_t stream);
extern "C" void afv_launch_vt_doc_count(const int *leaf, long long n, const int *image_ptr, int nimages, unsigned long long *table,
                                        unsigned long long table_mask, int *ni, hipStream_t stream);
