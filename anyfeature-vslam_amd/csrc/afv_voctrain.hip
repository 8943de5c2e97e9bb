// afv_voctrain.hip — host runtime of afv_vocab_train / afv_vocab_train_device (include/afv_hip.h; kernels: k_voctrain.hip).
// DBoW2 TemplatedVocabulary::create restated from upstream DBoW2 (the reference's DBoW2 is an empty submodule: parity unpinned); the
// normative restatement is tests/_voctrain_ref.py.  The tree is trained level by level - the generator key of a node is a function of the
// seed and its path, so nothing depends on the order in which nodes are worked - and renumbered to DBoW2's depth-first ids at the end.
#include <chrono>
#include <memory>

#include "afv_runtime.h"
#include "afv_voctrain.h"

struct afv_vocab_tree {
    int k = 0, L = 0, desc_bytes = 0, nnodes = 0;
    std::vector<int32_t> parent, ni, rounds;
    std::vector<uint8_t> desc, is_leaf;
    std::vector<double> weight, seconds;
    std::vector<int64_t> rows;
    int capped = 0;
};

namespace {

static unsigned long long sm64(unsigned long long x) {  // splitmix64
    x += 0x9E3779B97F4A7C15ull;
    unsigned long long z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct DevPool {  // device allocations of one call: freed together, on every way out
    std::vector<void *> p;
    ~DevPool() {
        for (void *q : p) (void)hipFree(q);
    }
    template <class T>
    hipError_t get(T **out, size_t count) {
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) p.push_back(q);
        *out = static_cast<T *>(q);
        return e;
    }
    void release(void *q) {
        for (size_t i = 0; i < p.size(); ++i)
            if (p[i] == q) {
                (void)hipFree(q);
                p.erase(p.begin() + (long)i);
                return;
            }
    }
};

struct OpenNode {
    int start, len, tmp;  // segment, id in creation (level) order
    unsigned long long key;
};

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static int validate(afv_ctx *c, const afv_vocab_train_params *p, const void *desc, int64_t n, const int32_t *image_ptr, int nimages, afv_vocab_tree **out) {
    if (out) *out = nullptr;
    if (!c || !p || !out || !desc || !image_ptr) return AFV_EINVAL;
    if (p->struct_size < sizeof(afv_vocab_train_params)) return AFV_EINVAL;
    if (p->k < 2 || p->k > 32 || p->L < 1 || p->L > 10 || p->desc_bytes < 1 || p->desc_bytes > 64 || p->max_iters < 0) return AFV_EINVAL;
    if (n < 1 || n > AFV_VOCAB_TRAIN_MAX_ROWS || nimages < 1) return AFV_EINVAL;
    if (p->init_centres ? (p->n_init < 1 || p->n_init > p->k) : p->n_init != 0) return AFV_EINVAL;
    if (image_ptr[0] != 0 || (int64_t)image_ptr[nimages] != n) return AFV_EINVAL;
    for (int i = 0; i < nimages; ++i)
        if (image_ptr[i + 1] < image_ptr[i]) return AFV_EINVAL;
    return AFV_OK;
}

// d_src: device rows at `pitch` bytes
static int train_impl(afv_ctx *c, const afv_vocab_train_params &prm, const uint8_t *d_src, size_t pitch, int n, const int32_t *image_ptr, int nimages,
                      afv_vocab_tree **out) {
    const int k = prm.k, L = prm.L, DB = prm.desc_bytes, W = DB <= 32 ? 8 : 16;
    hipStream_t st = c->stream;
    HIPCHK(c, hipSetDevice(c->device));
    if (!afv_voctrain_prepare()) {
        c->last_error = "afv_vocab_train: the association kernel cannot get its LDS";
        return AFV_EHIP;
    }
    DevPool pool;
    uint32_t *d_rows = nullptr, *d_rows2 = nullptr;
    uint8_t *d_assign = nullptr;
    int32_t *d_mindist = nullptr;
    int *d_status = nullptr;
    HIPCHK(c, pool.get(&d_rows, (size_t)n * W));
    HIPCHK(c, pool.get(&d_rows2, (size_t)n * W));
    HIPCHK(c, pool.get(&d_assign, (size_t)n));
    HIPCHK(c, pool.get(&d_mindist, (size_t)n));
    HIPCHK(c, pool.get(&d_status, 2));
    HIPCHK(c, hipMemsetAsync(d_status, 0, 8, st));
    afv_launch_vt_pad(d_src, pitch, DB, n, W, d_rows, st);
    HIPCHK(c, hipGetLastError());

    // the tree in creation order: node 0 = the root, the children of a node consecutive
    std::vector<int> t_parent{0}, t_first{-1}, t_nc{0};
    std::vector<uint32_t> t_desc((size_t)W, 0);
    auto tree = std::unique_ptr<afv_vocab_tree>(new afv_vocab_tree());
    tree->k = k, tree->L = L, tree->desc_bytes = DB;
    tree->rounds.assign((size_t)L, 0);
    tree->rows.assign((size_t)L, 0);
    tree->seconds.assign((size_t)L, 0.0);

    std::vector<OpenNode> open{{0, n, 0, sm64(prm.seed)}};
    for (int level = 1; level <= L && !open.empty(); ++level) {
        const double t0 = now_s();
        const int nn = (int)open.size();
        std::vector<VtNode> nodes((size_t)nn);
        std::vector<VtTile> tiles;
        std::vector<int> multi;
        int64_t work_rows = 0;
        for (int b = 0; b < nn; ++b) {
            VtNode &nd = nodes[(size_t)b];
            nd.start = open[(size_t)b].start, nd.len = open[(size_t)b].len, nd.key = open[(size_t)b].key, nd.pad = 0;
            nd.tile0 = (int)tiles.size();
            for (int o = 0; o < nd.len; o += VT_TILE) tiles.push_back(VtTile{b, nd.start + o, std::min(VT_TILE, nd.len - o)});
            nd.ntiles = (int)tiles.size() - nd.tile0;
            nd.slot = -1;
            if (nd.ntiles > 1) nd.slot = (int)multi.size(), multi.push_back(b);
            if (nd.len > k) work_rows += nd.len;
        }
        tree->rows[(size_t)level - 1] = work_rows;
        const int ntiles = (int)tiles.size(), nmulti = (int)multi.size(), bits = W * 32;
        DevPool lp;  // the level's arrays
        VtArgs a{};
        VtTile *d_tiles = nullptr;
        VtNode *d_nodes = nullptr;
        int *d_multi = nullptr, *d_flags = nullptr;
        HIPCHK(c, lp.get(&d_tiles, (size_t)ntiles));
        HIPCHK(c, lp.get(&d_nodes, (size_t)nn));
        HIPCHK(c, lp.get(&d_multi, (size_t)nmulti));
        HIPCHK(c, lp.get(&a.centres, (size_t)nn * k * W));
        HIPCHK(c, lp.get(&d_flags, (size_t)nn * (4 + k)));  // ncent | done | seeded | changed | sizes
        HIPCHK(c, lp.get(&a.gcnt, (size_t)nmulti * bits * k));
        HIPCHK(c, lp.get(&a.gsize, (size_t)nmulti * k));
        HIPCHK(c, lp.get(&a.tile_sum, (size_t)ntiles));
        HIPCHK(c, lp.get(&a.tile_hist, (size_t)ntiles * k));
        HIPCHK(c, lp.get(&a.tile_off, (size_t)ntiles * k));
        a.tiles = d_tiles, a.nodes = d_nodes, a.multi = d_multi;
        a.ntiles = ntiles, a.nnodes = nn, a.nmulti = nmulti, a.k = k, a.words = W;
        a.rows = d_rows, a.rows_out = d_rows2, a.assign = d_assign, a.mindist = d_mindist;
        a.ncent = d_flags, a.done = d_flags + nn, a.seeded = d_flags + 2 * (size_t)nn, a.changed = d_flags + 3 * (size_t)nn, a.sizes = d_flags + 4 * (size_t)nn;
        a.status = d_status;
        a.max_iters = prm.max_iters;
        HIPCHK(c, hipMemcpyAsync(d_tiles, tiles.data(), tiles.size() * sizeof(VtTile), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_nodes, nodes.data(), nodes.size() * sizeof(VtNode), hipMemcpyHostToDevice, st));
        if (nmulti) HIPCHK(c, hipMemcpyAsync(d_multi, multi.data(), multi.size() * sizeof(int), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemsetAsync(d_flags, 0, (size_t)nn * (4 + k) * sizeof(int), st));
        if (nmulti) {
            HIPCHK(c, hipMemsetAsync(a.gcnt, 0, (size_t)nmulti * bits * k * 4, st));
            HIPCHK(c, hipMemsetAsync(a.gsize, 0, (size_t)nmulti * k * 4, st));
        }
        std::vector<uint32_t> init_rows;
        if (level == 1 && prm.init_centres && n > k) {  // a warm start of the root: its seeding is replaced
            init_rows.assign((size_t)prm.n_init * W, 0);
            for (int i = 0; i < prm.n_init; ++i) std::memcpy(init_rows.data() + (size_t)i * W, prm.init_centres + (size_t)i * DB, (size_t)DB);
            const int preset[1] = {prm.n_init}, one[1] = {1};
            HIPCHK(c, hipMemcpyAsync(a.centres, init_rows.data(), init_rows.size() * 4, hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemcpyAsync(a.ncent, preset, 4, hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemcpyAsync(a.seeded, one, 4, hipMemcpyHostToDevice, st));
            HIPCHK(c, hipStreamSynchronize(st));  // (the sources are locals)
        }
        afv_launch_vt_seed_first(&a, st);
        if (work_rows > 0) {
            for (int draw = 1; draw < k; ++draw) {
                a.draw = draw;
                afv_launch_vt_seed_draw(&a, st);
            }
            HIPCHK(c, hipGetLastError());
            for (int round = 1;; ++round) {
                a.round = round;
                HIPCHK(c, hipMemsetAsync(d_status, 0, 4, st));  // (the capped flag next to it is sticky)
                afv_launch_vt_round(&a, st);
                HIPCHK(c, hipGetLastError());
                int status[2] = {0, 0};
                HIPCHK(c, hipMemcpyAsync(status, d_status, 8, hipMemcpyDeviceToHost, st));
                HIPCHK(c, hipStreamSynchronize(st));
                tree->rounds[(size_t)level - 1] = round;
                tree->capped = status[1] ? 1 : tree->capped;
                if (status[0] == 0) break;
            }
        }
        // the level's clusters become nodes: one per cluster (empty ones too), before anything below them
        std::vector<int> flags((size_t)nn * (4 + k));
        std::vector<uint32_t> cen((size_t)nn * k * W);
        HIPCHK(c, hipMemcpyAsync(flags.data(), d_flags, flags.size() * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(cen.data(), a.centres, cen.size() * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        std::vector<OpenNode> next;
        const int *ncent = flags.data(), *sizes = flags.data() + 4 * (size_t)nn;
        for (int b = 0; b < nn; ++b) {
            const int tmp = open[(size_t)b].tmp, nc = ncent[b];
            if (nc < 1 || nc > k) {
                c->last_error = "afv_vocab_train: a node came back without centres";
                return AFV_EHIP;
            }
            t_first[(size_t)tmp] = (int)t_parent.size(), t_nc[(size_t)tmp] = nc;
            int off = open[(size_t)b].start, total = 0;
            for (int cc = 0; cc < nc; ++cc) {
                const int id = (int)t_parent.size(), sz = sizes[(size_t)b * k + cc];
                if (sz < 0 || sz > open[(size_t)b].len) {
                    c->last_error = "afv_vocab_train: inconsistent cluster sizes";
                    return AFV_EHIP;
                }
                t_parent.push_back(tmp), t_first.push_back(-1), t_nc.push_back(0);
                t_desc.insert(t_desc.end(), cen.begin() + ((size_t)b * k + cc) * W, cen.begin() + ((size_t)b * k + cc + 1) * W);
                if (level < L && sz > 1) next.push_back(OpenNode{off, sz, id, sm64(open[(size_t)b].key ^ (unsigned long long)(cc + 1))});
                off += sz, total += sz;
            }
            if (total != open[(size_t)b].len) {
                c->last_error = "afv_vocab_train: inconsistent cluster sizes";
                return AFV_EHIP;
            }
        }
        if (!next.empty()) {
            afv_launch_vt_partition(&a, st);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipStreamSynchronize(st));  // the level's arrays go away
            std::swap(d_rows, d_rows2);
        }
        open.swap(next);
        tree->seconds[(size_t)level - 1] = now_s() - t0;
    }

    // DBoW2's ids: HKmeansStep numbers all clusters of a node, then descends into them in order
    const int NN = (int)t_parent.size();
    std::vector<int> id_of((size_t)NN, -1), order;  // creation index -> DBoW2 id; DBoW2 id -> creation index
    order.reserve((size_t)NN);
    id_of[0] = 0, order.push_back(0);
    {
        std::vector<std::pair<int, int>> stack;  // (node, next child to descend into)
        auto number_children = [&](int t) {
            for (int q = 0; q < t_nc[(size_t)t]; ++q) id_of[(size_t)(t_first[(size_t)t] + q)] = (int)order.size(), order.push_back(t_first[(size_t)t] + q);
        };
        number_children(0);
        stack.push_back({0, 0});
        while (!stack.empty()) {
            auto &top = stack.back();
            if (top.second >= t_nc[(size_t)top.first]) {
                stack.pop_back();
                continue;
            }
            const int child = t_first[(size_t)top.first] + top.second++;
            if (t_nc[(size_t)child] > 0) {
                number_children(child);
                stack.push_back({child, 0});
            }
        }
    }
    tree->nnodes = NN;
    tree->parent.assign((size_t)NN, 0);
    tree->desc.assign((size_t)NN * DB, 0);
    tree->is_leaf.assign((size_t)NN, 0);
    tree->weight.assign((size_t)NN, 0.0);
    tree->ni.assign((size_t)NN, -1);
    for (int id = 0; id < NN; ++id) {
        const int t = order[(size_t)id];
        tree->parent[(size_t)id] = id_of[(size_t)t_parent[(size_t)t]];
        tree->is_leaf[(size_t)id] = id > 0 && t_nc[(size_t)t] == 0;
        std::memcpy(tree->desc.data() + (size_t)id * DB, t_desc.data() + (size_t)t * W, (size_t)DB);
    }
    // setNodeWeights (TF-IDF): descend the finished tree (k_bow.hip, the descent afv_bow_transform runs), count the images of every word
    std::vector<int32_t> child_ptr((size_t)NN + 1, 0), child_idx;
    child_idx.reserve((size_t)NN);
    for (int id = 0; id < NN; ++id) {
        const int t = order[(size_t)id];
        for (int q = 0; q < t_nc[(size_t)t]; ++q) child_idx.push_back(id_of[(size_t)(t_first[(size_t)t] + q)]);
        child_ptr[(size_t)id + 1] = (int32_t)child_idx.size();
    }
    afv_vocab *voc = nullptr;
    int rc = afv_vocab_create(c, k, L, NN, child_ptr.data(), child_idx.data(), tree->desc.data(), DB, &voc);
    if (rc != AFV_OK) return rc;
    struct VocGuard {
        afv_ctx *c;
        afv_vocab *v;
        ~VocGuard() { afv_vocab_destroy(c, v); }
    } guard{c, voc};
    pool.release(d_rows2);
    d_rows2 = nullptr;
    int *d_leaf = nullptr, *d_nid = nullptr, *d_ni = nullptr, *d_iptr = nullptr;
    unsigned long long *d_table = nullptr;
    size_t slots = 1024;
    while (slots < 2 * (size_t)n) slots <<= 1;
    HIPCHK(c, pool.get(&d_leaf, (size_t)n));
    HIPCHK(c, pool.get(&d_nid, (size_t)n));
    HIPCHK(c, pool.get(&d_ni, (size_t)NN));
    HIPCHK(c, pool.get(&d_iptr, (size_t)nimages + 1));
    HIPCHK(c, pool.get(&d_table, slots));
    HIPCHK(c, hipMemsetAsync(d_ni, 0, (size_t)NN * 4, st));
    HIPCHK(c, hipMemsetAsync(d_table, 0xff, slots * 8, st));
    HIPCHK(c, hipMemcpyAsync(d_iptr, image_ptr, ((size_t)nimages + 1) * 4, hipMemcpyHostToDevice, st));
    afv_launch_vt_pad(d_src, pitch, DB, n, W, d_rows, st);  // the rows in their original order again
    afv_launch_bow_transform(&voc->dev, d_rows, n, 0, d_leaf, d_nid, nullptr, st);
    afv_launch_vt_doc_count(d_leaf, n, d_iptr, nimages, d_table, (unsigned long long)slots - 1, d_ni, st);
    HIPCHK(c, hipGetLastError());
    std::vector<int> ni((size_t)NN);
    HIPCHK(c, hipMemcpyAsync(ni.data(), d_ni, (size_t)NN * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    for (int id = 0; id < NN; ++id) {
        if (!tree->is_leaf[(size_t)id]) continue;
        tree->ni[(size_t)id] = ni[(size_t)id];
        if (ni[(size_t)id] > 0) tree->weight[(size_t)id] = std::log((double)nimages / (double)ni[(size_t)id]);
    }
    *out = tree.release();
    return AFV_OK;
}

}  // namespace

extern "C" int afv_vocab_train_device(afv_ctx *c, const afv_vocab_train_params *params, const uint8_t *d_desc, size_t pitch_bytes, int64_t n,
                                      const int32_t *image_ptr, int nimages, afv_vocab_tree **out) {
    const int rc = validate(c, params, d_desc, n, image_ptr, nimages, out);
    if (rc != AFV_OK) return rc;
    if (pitch_bytes < (size_t)params->desc_bytes) return AFV_EINVAL;
    return guarded(c, [&]() -> int { return train_impl(c, *params, d_desc, pitch_bytes, (int)n, image_ptr, nimages, out); });
}

extern "C" int afv_vocab_train(afv_ctx *c, const afv_vocab_train_params *params, const uint8_t *desc, int64_t n, const int32_t *image_ptr, int nimages,
                               afv_vocab_tree **out) {
    const int rc = validate(c, params, desc, n, image_ptr, nimages, out);
    if (rc != AFV_OK) return rc;
    return guarded(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        DevPool pool;
        uint8_t *d_src = nullptr;
        const size_t bytes = (size_t)n * params->desc_bytes;
        HIPCHK(c, pool.get(&d_src, bytes));
        HIPCHK(c, hipMemcpyAsync(d_src, desc, bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return train_impl(c, *params, d_src, (size_t)params->desc_bytes, (int)n, image_ptr, nimages, out);
    });
}

extern "C" int afv_vocab_tree_nnodes(const afv_vocab_tree *t) { return t ? t->nnodes : AFV_EINVAL; }

extern "C" int afv_vocab_tree_get(const afv_vocab_tree *t, int32_t *parent, uint8_t *desc, uint8_t *is_leaf, double *weight, int32_t *ni) {
    if (!t) return AFV_EINVAL;
    if (parent) std::memcpy(parent, t->parent.data(), t->parent.size() * sizeof(int32_t));
    if (desc) std::memcpy(desc, t->desc.data(), t->desc.size());
    if (is_leaf) std::memcpy(is_leaf, t->is_leaf.data(), t->is_leaf.size());
    if (weight) std::memcpy(weight, t->weight.data(), t->weight.size() * sizeof(double));
    if (ni) std::memcpy(ni, t->ni.data(), t->ni.size() * sizeof(int32_t));
    return AFV_OK;
}

extern "C" int afv_vocab_tree_stats(const afv_vocab_tree *t, int32_t *rounds, int64_t *rows, double *seconds, int32_t *capped) {
    if (!t) return AFV_EINVAL;
    if (rounds) std::memcpy(rounds, t->rounds.data(), t->rounds.size() * sizeof(int32_t));
    if (rows) std::memcpy(rows, t->rows.data(), t->rows.size() * sizeof(int64_t));
    if (seconds) std::memcpy(seconds, t->seconds.data(), t->seconds.size() * sizeof(double));
    if (capped) *capped = t->capped;
    return AFV_OK;
}

extern "C" void afv_vocab_tree_destroy(afv_vocab_tree *t) { delete t; }
