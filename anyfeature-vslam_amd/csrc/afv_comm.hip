// afv_comm.hip — keyframe descriptor table resident in HBM and its multi-GPU replication (BASELINE.json configs[3]).
//
// Reference call shape: LoopClosing::ComputeSim3 (src/LoopClosing.cc:255-281) runs SearchByBoW(KF,KF) once per loop
// candidate returned by KeyFrameDatabase::DetectLoopCandidates (src/KeyFrameDatabase.cc:76-197); Tracking::Relocalization
// (src/Tracking.cc:1162-1182) does the same per relocalisation candidate; LocalMapping::CreateNewMapPoints
// (src/LocalMapping.cc:238-297) runs SearchForTriangulation against <= 20 neighbours.  Every call re-reads descriptors
// that are const after keyframe construction (include/KeyFrame.h:190).  Here they are uploaded ONCE into a table
// [nsets][cap][pitch] and batches of (a, b) jobs run against it; only pair lists go in and match vectors come out.  Binary descriptors of
// 1 to 64 bytes: rows zero-padded to a pitch of 32 bytes (up to 32-byte descriptors) or 64 bytes (33 to 64), the rule of resident frames;
// the padding is zero on both sides of every distance, so it adds nothing.  Float descriptors (afv_table_create_f32: SIFT128, SURF64,
// KAZE64 ...): rows of float_dim floats without padding, the fields of a resident float frame (desc_bytes = 4 * float_dim, words =
// float_dim); the distance is L2^2 as cv::norm evaluates it (k_match_l2.hip, the W == 0 instantiations of k_match.hip).
//
// Multi-GPU: one process per GPU; the table is replicated with ONE ncclBroadcast per array (RCCL over
// xGMI), jobs are block-partitioned (afv_shard_range), no other data-path collective exists.  RCCL is resolved at run
// time (dlopen / already-loaded copy), so libafv_hip.so carries no link dependency on it and single-GPU hosts never
// touch it.
#include <dlfcn.h>
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#else
// hosts without the RCCL development headers: the few declarations this file needs (the library is resolved with dlopen at run time)
extern "C" {
typedef struct ncclComm *ncclComm_t;
#define NCCL_UNIQUE_ID_BYTES 128
typedef struct { char internal[NCCL_UNIQUE_ID_BYTES]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclInt8 = 0, ncclChar = 0, ncclUint8 = 1 } ncclDataType_t;
}
#endif

#include <mutex>

#include "afv_runtime.h"

// ------------------------------------------------------------------------------------------------------------------
// table
// ------------------------------------------------------------------------------------------------------------------
struct afv_comm {
    afv_ctx *c = nullptr;
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;
};

static std::mutex g_reg_mutex;
static std::vector<afv_table *> g_tables;
static std::vector<afv_comm *> g_comms;

static void table_free(afv_table *t) {
    if (!t) return;
    if (t->c) (void)hipSetDevice(t->c->device);
    void *ptrs[] = {t->d_desc, t->d_angle, t->d_n, t->d_idx, t->d_geo, t->d_scale, t->d_inf, t->d_valid, t->d_pairs, t->d_out, t->d_nm, t->d_bow_word, t->d_bow_value, t->d_bow_n};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    afv_kffuse_free(t);
    if (t->h_pin) (void)hipHostFree(t->h_pin);
    if (t->ev0) (void)hipEventDestroy(t->ev0);
    if (t->ev1) (void)hipEventDestroy(t->ev1);
    delete t;
}

static inline size_t table_pitch(const afv_table *t) { return (size_t)t->words * 4; }

static int table_create(afv_ctx *c, int nsets, int cap, int desc_bytes, afv_table **out, int float_dim = 0) {
    if (!c || !out || nsets < 1 || cap < 1 || cap > 4096) return AFV_EINVAL;
    *out = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    afv_table *t = new (std::nothrow) afv_table();
    if (!t) return AFV_ENOMEM;
    t->c = c;
    t->nsets = nsets;
    t->cap = cap;
    t->desc_bytes = desc_bytes;
    t->words = float_dim ? float_dim : (desc_bytes <= 32 ? 8 : 16);
    t->float_dim = float_dim;
    hipError_t e = hipMalloc(&t->d_desc, (size_t)nsets * cap * table_pitch(t));
    // rows narrower than their pitch: the padding starts (and, since every writer writes whole padded rows, stays) zero
    if (e == hipSuccess && (size_t)desc_bytes != table_pitch(t)) e = afv_fill(c, t->d_desc, 0, (size_t)nsets * cap * table_pitch(t));
    if (e == hipSuccess) e = hipMalloc(&t->d_angle, (size_t)nsets * cap * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&t->d_n, (size_t)nsets * sizeof(int32_t));
    if (e == hipSuccess) e = afv_fill(c, t->d_n, 0, (size_t)nsets * sizeof(int32_t));
    if (e == hipSuccess) e = afv_fill(c, t->d_angle, 0, (size_t)nsets * cap * sizeof(float));
    if (e == hipSuccess) e = hipEventCreate(&t->ev0);
    if (e == hipSuccess) e = hipEventCreate(&t->ev1);
    if (e != hipSuccess) {
        c->last_error = std::string("afv_table_create: ") + hipGetErrorString(e);
        table_free(t);
        return e == hipErrorOutOfMemory ? AFV_ENOMEM : AFV_EHIP;
    }
    try {
        t->h_n.assign((size_t)nsets, 0);
        t->fv.resize((size_t)nsets);
        t->has_fv.assign((size_t)nsets, 0);
        t->has_geo.assign((size_t)nsets, 0);
        t->has_scale.assign((size_t)nsets, 0);
        t->has_inf.assign((size_t)nsets, 0);
        t->h_bow_n.assign((size_t)nsets, 0);
        t->has_bow.assign((size_t)nsets, 0);
        t->fv_body_on_device.assign((size_t)nsets, 0);
        std::lock_guard<std::mutex> g(g_reg_mutex);
        g_tables.push_back(t);
    } catch (...) {
        table_free(t);
        return AFV_ENOMEM;
    }
    *out = t;
    return AFV_OK;
}

extern "C" int afv_table_create(afv_ctx *c, int nsets, int cap, afv_table **out) { return table_create(c, nsets, cap, AFV_DESC_BYTES, out); }

extern "C" int afv_table_create_bytes(afv_ctx *c, int nsets, int cap, int desc_bytes, afv_table **out) {
    if (desc_bytes < 1 || desc_bytes > 64) return AFV_EINVAL;
    return table_create(c, nsets, cap, desc_bytes, out);
}

extern "C" int afv_table_create_f32(afv_ctx *c, int nsets, int cap, int float_dim, afv_table **out) {
    if (float_dim < 4 || float_dim > 1024 || (float_dim & 3)) return AFV_EINVAL;  // the rule of afv_frame_params.float_dim
    return table_create(c, nsets, cap, 4 * float_dim, out, float_dim);
}

extern "C" void afv_table_destroy(afv_table *t) {
    if (!t) return;
    {
        std::lock_guard<std::mutex> g(g_reg_mutex);
        auto it = std::find(g_tables.begin(), g_tables.end(), t);
        if (it == g_tables.end()) return;  // already released with its context
        g_tables.erase(it);
    }
    if (t->c) {
        (void)hipSetDevice(t->c->device);
        (void)hipStreamSynchronize(t->c->stream);
        (void)hipStreamSynchronize(t->c->stream2);
    }
    table_free(t);
}

extern "C" int afv_table_set(afv_table *t, int set, const uint8_t *desc32, const float *angles, int n) {
    if (!t || set < 0 || set >= t->nsets || n < 0 || n > t->cap || (n > 0 && !desc32)) return AFV_EINVAL;
    afv_ctx *c = t->c;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t pitch = table_pitch(t);
    if (n && (size_t)t->desc_bytes == pitch) {
        HIPCHK(c, hipMemcpyAsync(t->d_desc + (size_t)set * t->cap * pitch, desc32, (size_t)n * pitch, hipMemcpyHostToDevice, c->stream));
    } else if (n) {  // rows of desc_bytes -> zero-padded rows of the pitch (the stream is synchronised below: the staging outlives the copy)
        std::vector<uint8_t> rows((size_t)n * pitch, 0);
        for (int i = 0; i < n; ++i) std::memcpy(rows.data() + (size_t)i * pitch, desc32 + (size_t)i * t->desc_bytes, (size_t)t->desc_bytes);
        HIPCHK(c, hipMemcpyAsync(t->d_desc + (size_t)set * t->cap * pitch, rows.data(), rows.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (n && angles)
        HIPCHK(c, hipMemcpyAsync(t->d_angle + (size_t)set * t->cap, angles, (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    else if (n)
        HIPCHK(c, hipMemsetAsync(t->d_angle + (size_t)set * t->cap, 0, (size_t)n * sizeof(float), c->stream));
    t->h_n[set] = n;
    // a recycled slot must not inherit anything of its previous occupant: FeatureVector (indices may be out of range), "map point
    // exists" mask (unset = all valid), geometry (afv_table_match_triangulation refuses the slot until it is set again)
    t->fv[set] = HostFeatVec();
    t->has_fv[set] = 0;
    t->fv_body_on_device[set] = 0;
    t->has_geo[set] = 0;
    t->has_scale[set] = 0;
    t->has_inf[set] = 0;
    t->has_bow[set] = 0;
    t->h_bow_n[set] = 0;
    afv_kffuse_slot_reset(t, set);
    if (t->d_bow_n) HIPCHK(c, hipMemsetAsync(t->d_bow_n + set, 0, sizeof(int32_t), c->stream));
    if (t->d_valid) HIPCHK(c, hipMemsetAsync(t->d_valid + (size_t)set * t->cap, 1, (size_t)t->cap, c->stream));
    HIPCHK(c, hipMemcpyAsync(t->d_n + set, &t->h_n[set], sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AFV_OK;
}

extern "C" int afv_table_set_featvec(afv_table *t, int set, const int32_t *node_id, const int32_t *seg_ptr, const int32_t *seg_idx,
                                     int nnodes) {
    if (!t || set < 0 || set >= t->nsets || nnodes < 0 || (nnodes > 0 && (!node_id || !seg_ptr || !seg_idx))) return AFV_EINVAL;
    afv_ctx *c = t->c;
    const int n = t->h_n[set];
    if (afv_featvec_check(node_id, seg_ptr, seg_idx, nnodes, n)) return AFV_EINVAL;
    const int total = nnodes ? seg_ptr[nnodes] : 0;
    return guarded(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        if (!t->d_idx) HIPCHK(c, hipMalloc(&t->d_idx, (size_t)t->nsets * t->cap * sizeof(int32_t)));
        HostFeatVec &f = t->fv[set];
        f.node_id.assign(node_id, node_id + nnodes);
        f.seg_ptr.assign(seg_ptr, seg_ptr + (nnodes ? nnodes + 1 : 0));
        f.seg_idx.assign(seg_idx, seg_idx + total);
        t->fv_body_on_device[set] = 0;
        if (total) HIPCHK(c, hipMemcpy(t->d_idx + (size_t)set * t->cap, seg_idx, (size_t)total * sizeof(int32_t), hipMemcpyHostToDevice));
        t->has_fv[set] = 1;
        return AFV_OK;
    });
}

extern "C" int afv_table_set_geometry(afv_table *t, int set, const float *x, const float *y, const float *sigma2) {
    if (!t || set < 0 || set >= t->nsets || !x || !y || !sigma2) return AFV_EINVAL;
    afv_ctx *c = t->c;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t plane = (size_t)t->nsets * t->cap;
    if (!t->d_geo) HIPCHK(c, hipMalloc(&t->d_geo, 4 * plane * sizeof(float)));
    const int n = t->h_n[set];
    t->has_geo[set] = 1;
    afv_kffuse_grid_stale(t, set);
    if (n == 0) return AFV_OK;
    const std::vector<float> mono((size_t)n, -1.0f);  // a keyframe is monocular until afv_table_set_u_right says otherwise
    const float *src[4] = {x, y, sigma2, mono.data()};
    for (int k = 0; k < 4; ++k)
        HIPCHK(c, hipMemcpy(t->d_geo + k * plane + (size_t)set * t->cap, src[k], (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    return AFV_OK;
}

extern "C" int afv_table_set_u_right(afv_table *t, int set, const float *u_right) {
    if (!t || set < 0 || set >= t->nsets || !u_right) return AFV_EINVAL;
    if (!t->d_geo || !t->has_geo[set]) return AFV_EINVAL;  // after afv_table_set_geometry of the same slot
    afv_ctx *c = t->c;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t plane = (size_t)t->nsets * t->cap;
    const int n = t->h_n[set];
    if (n > 0) HIPCHK(c, hipMemcpy(t->d_geo + 3 * plane + (size_t)set * t->cap, u_right, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    return AFV_OK;
}

// GetKeyPt2DInf of a slot: what OptimizeSim3 reads next to the geometry (afv_table_optimize_sim3)
extern "C" int afv_table_set_inf(afv_table *t, int set, const float *inf) {
    if (!t || set < 0 || set >= t->nsets || !inf) return AFV_EINVAL;
    if (!t->d_geo || !t->has_geo[set]) return AFV_EINVAL;  // after afv_table_set_geometry of the same slot
    afv_ctx *c = t->c;
    return guarded(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        if (!t->d_inf) HIPCHK(c, hipMalloc(&t->d_inf, (size_t)t->nsets * t->cap * sizeof(float)));
        const int n = t->h_n[set];
        t->has_inf[set] = 1;
        if (n > 0) HIPCHK(c, hipMemcpy(t->d_inf + (size_t)set * t->cap, inf, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
        return AFV_OK;
    });
}

// keyPtsSize, mvDepth and the distorted mvKeys of a slot: what CreateNewMapPoints reads next to the geometry (afv_table_triangulate)
extern "C" int afv_table_set_scale(afv_table *t, int set, const float *size, const float *depth, const float *x_dist, const float *y_dist) {
    if (!t || set < 0 || set >= t->nsets || !size || (!x_dist != !y_dist)) return AFV_EINVAL;
    if (!t->d_geo || !t->has_geo[set]) return AFV_EINVAL;  // after afv_table_set_geometry of the same slot
    afv_ctx *c = t->c;
    return guarded(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        const size_t plane = (size_t)t->nsets * t->cap, row0 = (size_t)set * t->cap;
        if (!t->d_scale) HIPCHK(c, hipMalloc(&t->d_scale, 4 * plane * sizeof(float)));
        const int n = t->h_n[set];
        t->has_scale[set] = 1;
        afv_kffuse_grid_stale(t, set);
        if (n == 0) return AFV_OK;
        const std::vector<float> none((size_t)n, -1.0f);  // mvDepth of a monocular keyframe
        HIPCHK(c, hipMemcpy(t->d_scale + row0, size, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(t->d_scale + plane + row0, depth ? depth : none.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice));
        for (int k = 0; k < 2; ++k) {  // no distortion: mvKeys == mvKeysUn
            const float *src = k ? y_dist : x_dist;
            if (src) HIPCHK(c, hipMemcpy(t->d_scale + (2 + k) * plane + row0, src, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
            else HIPCHK(c, afv_copy_dd(c, t->d_scale + (2 + k) * plane + row0, t->d_geo + k * plane + row0, (size_t)n * sizeof(float)));
        }
        return AFV_OK;
    });
}

extern "C" int afv_table_set_valid(afv_table *t, int set, const uint8_t *valid) {
    if (!t || set < 0 || set >= t->nsets) return AFV_EINVAL;
    afv_ctx *c = t->c;
    HIPCHK(c, hipSetDevice(c->device));
    if (!t->d_valid) {
        if (!valid) return AFV_OK;  // nothing was ever restricted
        HIPCHK(c, hipMalloc(&t->d_valid, (size_t)t->nsets * t->cap));
        HIPCHK(c, afv_fill(c, t->d_valid, 1, (size_t)t->nsets * t->cap));
    }
    const int n = t->h_n[set];
    if (valid) {
        if (n) HIPCHK(c, hipMemcpy(t->d_valid + (size_t)set * t->cap, valid, (size_t)n, hipMemcpyHostToDevice));
    } else {
        HIPCHK(c, afv_fill(c, t->d_valid + (size_t)set * t->cap, 1, (size_t)t->cap));
    }
    return AFV_OK;
}

// BowVector planes: allocated together on first use, counts zero
static int table_ensure_bow(afv_table *t) {
    if (t->d_bow_word) return AFV_OK;
    afv_ctx *c = t->c;
    const size_t plane = (size_t)t->nsets * t->cap;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&t->d_bow_word), plane * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&t->d_bow_value), plane * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&t->d_bow_n), (size_t)t->nsets * sizeof(int32_t));
    if (e == hipSuccess) e = afv_fill(c, t->d_bow_n, 0, (size_t)t->nsets * sizeof(int32_t));
    if (e != hipSuccess) {
        for (void *p : {(void *)t->d_bow_word, (void *)t->d_bow_value, (void *)t->d_bow_n})
            if (p) (void)hipFree(p);
        t->d_bow_word = t->d_bow_n = nullptr;
        t->d_bow_value = nullptr;
    }
    HIPCHK(c, e);
    return AFV_OK;
}

extern "C" int afv_table_set_bowvec(afv_table *t, int set, const int32_t *word, const double *value, int n) {
    if (!t || set < 0 || set >= t->nsets || n < 0 || n > t->cap || (n > 0 && (!word || !value))) return AFV_EINVAL;
    for (int i = 0; i < n; ++i)
        if (word[i] < 0 || (i > 0 && word[i] <= word[i - 1])) return AFV_EINVAL;  // ascending and unique: what the score kernel searches
    afv_ctx *c = t->c;
    return guarded(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        const int rc = table_ensure_bow(t);
        if (rc) return rc;
        const int32_t n32 = n;
        if (n) {
            HIPCHK(c, hipMemcpyAsync(t->d_bow_word + (size_t)set * t->cap, word, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(t->d_bow_value + (size_t)set * t->cap, value, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        }
        HIPCHK(c, hipMemcpyAsync(t->d_bow_n + set, &n32, sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // the sources were pageable
        t->h_bow_n[set] = n;
        t->has_bow[set] = 1;
        return AFV_OK;
    });
}

extern "C" int afv_table_device_ptrs(afv_table *t, uint8_t **d_desc, float **d_angle, int32_t **d_n) {
    if (!t) return AFV_EINVAL;
    if (d_desc) *d_desc = t->d_desc;
    if (d_angle) *d_angle = t->d_angle;
    if (d_n) *d_n = t->d_n;
    return AFV_OK;
}

extern "C" int afv_table_sync_counts(afv_table *t) {  // after a broadcast / external device-side write of d_n
    if (!t) return AFV_EINVAL;
    afv_ctx *c = t->c;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<int32_t> fresh((size_t)t->nsets);
    HIPCHK(c, hipMemcpy(fresh.data(), t->d_n, (size_t)t->nsets * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int s = 0; s < t->nsets; ++s) {
        const int v = std::min(std::max(fresh[s], 0), t->cap);
        if (v < t->h_n[s] && t->has_fv[s]) {
            // the set shrank under a stored FeatureVector: indices >= v would address rows that no longer exist
            bool stale = t->fv_body_on_device[s] != 0;  // (a promoted frame's body has no host copy to check: dropped with the shrink)
            for (int32_t i : t->fv[s].seg_idx) stale |= i >= v;
            if (stale) {
                t->fv[s] = HostFeatVec();
                t->has_fv[s] = 0;
                t->fv_body_on_device[s] = 0;
            }
        }
        t->h_n[s] = v;
    }
    afv_kffuse_grid_stale(t, -1);
    return AFV_OK;
}

// ---- replica image: everything a replica needs besides the device planes (host-side FeatureVector structure + per-set flags).
// Layout (int32): [nsets] then per set {has_fv, has_geo | has_scale << 1 | has_inf << 2, has_bow, bow_n, nnodes, node_id[nnodes], seg_ptr[nnodes + 1] (absent when nnodes == 0)}.
// The feature indices themselves travel with the d_idx plane, the BowVector entries with the BowVector planes. ----
static void table_pack_meta(const afv_table *t, std::vector<int32_t> &blob) {
    blob.clear();
    blob.push_back(t->nsets);
    for (int s = 0; s < t->nsets; ++s) {
        const HostFeatVec &f = t->fv[s];
        blob.push_back(t->has_fv[s]);
        blob.push_back(t->has_geo[s] | (t->has_scale[s] << 1) | (t->has_inf[s] << 2));  // bit 1: the scale planes (afv_table_set_scale), bit 2: the information plane (afv_table_set_inf)
        blob.push_back(t->has_bow[s]);
        blob.push_back(t->h_bow_n[s]);
        blob.push_back((int32_t)f.node_id.size());
        blob.insert(blob.end(), f.node_id.begin(), f.node_id.end());
        blob.insert(blob.end(), f.seg_ptr.begin(), f.seg_ptr.end());
    }
}

// rebuilds fv[] / flags of `t` from a replica image; the d_idx plane and the counts (h_n) must already be in place
static int table_unpack_meta(afv_table *t, const int32_t *blob, size_t len) {
    afv_ctx *c = t->c;
    if (len < 1 || blob[0] != t->nsets) return AFV_EINVAL;
    size_t pos = 1;
    std::vector<int32_t> idx_row((size_t)t->cap);
    for (int s = 0; s < t->nsets; ++s) {
        if (pos + 5 > len) return AFV_EINVAL;
        const int has_fv = blob[pos], has_geo = blob[pos + 1], has_bow = blob[pos + 2], bow_n = blob[pos + 3], nnodes = blob[pos + 4];
        pos += 5;
        if (bow_n < 0 || bow_n > t->cap || ((has_bow || bow_n) && !t->d_bow_word)) return AFV_EINVAL;
        if ((has_geo & 2) && !t->d_scale) return AFV_EINVAL;
        if ((has_geo & 4) && !t->d_inf) return AFV_EINVAL;
        if (nnodes < 0 || pos + (size_t)nnodes + (nnodes ? (size_t)nnodes + 1 : 0) > len) return AFV_EINVAL;
        HostFeatVec f;
        f.node_id.assign(blob + pos, blob + pos + nnodes);
        pos += (size_t)nnodes;
        if (nnodes) {
            f.seg_ptr.assign(blob + pos, blob + pos + nnodes + 1);
            pos += (size_t)nnodes + 1;
            const int total = f.seg_ptr[nnodes];
            if (total < 0 || total > t->h_n[s] || !t->d_idx) return AFV_EINVAL;
            if (total) {
                HIPCHK(c, hipMemcpy(idx_row.data(), t->d_idx + (size_t)s * t->cap, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost));
                f.seg_idx.assign(idx_row.begin(), idx_row.begin() + total);
            }
            if (afv_featvec_check(f.node_id.data(), f.seg_ptr.data(), f.seg_idx.data(), nnodes, t->h_n[s])) return AFV_EINVAL;
        }
        t->fv[s] = std::move(f);
        t->fv_body_on_device[s] = 0;
        t->has_fv[s] = has_fv != 0;
        t->has_geo[s] = (has_geo & 1) != 0;
        t->has_scale[s] = (has_geo & 2) != 0;
        t->has_inf[s] = (has_geo & 4) != 0;
        t->has_bow[s] = has_bow != 0;
        t->h_bow_n[s] = bow_n;
    }
    return pos == len ? AFV_OK : AFV_EINVAL;
}

extern "C" int afv_table_clone(const afv_table *src, afv_table *dst) {
    if (!src || !dst || src == dst || src->nsets != dst->nsets || src->cap != dst->cap) return AFV_EINVAL;
    // another kind or float dimension (the pitch does not tell: 64 bytes and 16 floats share one); two binary widths: AFV_EINVAL as before
    if (src->float_dim != dst->float_dim) return AFV_EUNSUPPORTED;
    if (src->desc_bytes != dst->desc_bytes) return AFV_EINVAL;
    afv_ctx *c = dst->c;
    return guarded(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(src->c->device));
        HIPCHK(c, hipStreamSynchronize(src->c->stream));
        HIPCHK(c, hipSetDevice(c->device));
        const size_t plane = (size_t)dst->nsets * dst->cap;
        if (src->d_idx && !dst->d_idx) HIPCHK(c, hipMalloc(&dst->d_idx, plane * sizeof(int32_t)));
        if (src->d_geo && !dst->d_geo) HIPCHK(c, hipMalloc(&dst->d_geo, 4 * plane * sizeof(float)));
        if (src->d_scale && !dst->d_scale) HIPCHK(c, hipMalloc(&dst->d_scale, 4 * plane * sizeof(float)));
        if (src->d_inf && !dst->d_inf) HIPCHK(c, hipMalloc(&dst->d_inf, plane * sizeof(float)));
        if (src->d_valid && !dst->d_valid) HIPCHK(c, hipMalloc(&dst->d_valid, plane));
        if (src->d_bow_word) {
            const int rcb = table_ensure_bow(dst);
            if (rcb) return rcb;
            HIPCHK(c, afv_copy_dd(c, dst->d_bow_word, src->d_bow_word, plane * sizeof(int32_t)));
            HIPCHK(c, afv_copy_dd(c, dst->d_bow_value, src->d_bow_value, plane * sizeof(double)));
            HIPCHK(c, afv_copy_dd(c, dst->d_bow_n, src->d_bow_n, (size_t)dst->nsets * sizeof(int32_t)));
        } else if (dst->d_bow_n) {
            HIPCHK(c, afv_fill(c, dst->d_bow_n, 0, (size_t)dst->nsets * sizeof(int32_t)));
        }
        HIPCHK(c, afv_copy_dd(c, dst->d_desc, src->d_desc, plane * table_pitch(dst)));
        HIPCHK(c, afv_copy_dd(c, dst->d_angle, src->d_angle, plane * sizeof(float)));
        HIPCHK(c, afv_copy_dd(c, dst->d_n, src->d_n, (size_t)dst->nsets * sizeof(int32_t)));
        if (src->d_idx) HIPCHK(c, afv_copy_dd(c, dst->d_idx, src->d_idx, plane * sizeof(int32_t)));
        if (src->d_geo) HIPCHK(c, afv_copy_dd(c, dst->d_geo, src->d_geo, 4 * plane * sizeof(float)));
        if (src->d_scale) HIPCHK(c, afv_copy_dd(c, dst->d_scale, src->d_scale, 4 * plane * sizeof(float)));
        if (src->d_inf) HIPCHK(c, afv_copy_dd(c, dst->d_inf, src->d_inf, plane * sizeof(float)));
        if (src->d_valid) HIPCHK(c, afv_copy_dd(c, dst->d_valid, src->d_valid, plane));
        else if (dst->d_valid) HIPCHK(c, afv_fill(c, dst->d_valid, 1, plane));
        for (int s = 0; s < dst->nsets; ++s) {  // nothing of the destination's previous content survives
            dst->fv[s] = HostFeatVec();
            dst->has_fv[s] = dst->has_geo[s] = dst->has_scale[s] = dst->has_inf[s] = dst->has_bow[s] = 0;
            dst->h_bow_n[s] = 0;
            dst->fv_body_on_device[s] = 0;
        }
        int rc = afv_table_sync_counts(dst);
        if (rc) return rc;
        std::vector<int32_t> blob;
        table_pack_meta(src, blob);
        rc = table_unpack_meta(dst, blob.data(), blob.size());  // the code path every receiver of afv_table_broadcast runs
        return rc ? rc : afv_kffuse_clone(src, dst);
    });
}

static int table_reserve_pairs(afv_table *t, int npairs) {
    afv_ctx *c = t->c;
    if (npairs <= t->pair_cap) return AFV_OK;
    HIPCHK(c, hipDeviceSynchronize());
    if (t->d_pairs) (void)hipFree(t->d_pairs);
    if (t->d_out) (void)hipFree(t->d_out);
    if (t->d_nm) (void)hipFree(t->d_nm);
    if (t->h_pin) (void)hipHostFree(t->h_pin);
    t->d_pairs = t->d_out = t->d_nm = nullptr;
    t->h_pin = nullptr;
    t->pair_cap = 0;
    const int want = npairs + npairs / 4;
    HIPCHK(c, hipMalloc(&t->d_pairs, (size_t)want * 2 * sizeof(int32_t)));
    HIPCHK(c, hipMalloc(&t->d_out, (size_t)want * t->cap * sizeof(int32_t)));
    HIPCHK(c, hipMalloc(&t->d_nm, (size_t)want * sizeof(int32_t)));
    HIPCHK(c, hipHostMalloc(reinterpret_cast<void **>(&t->h_pin), ((size_t)want * 3 + (size_t)want * t->cap) * sizeof(int32_t), hipHostMallocDefault));
    t->pair_cap = want;
    return AFV_OK;
}

// test hooks (afv_debug_scratch_bytes / _paint_scratch / _scratch_read): the buffers of table_reserve_pairs of every table of `c`.  Scratch
// by contract: afv_table_match_pairs uploads the pairs, the matcher writes d_out / d_nm, the call copies them out and nothing reads them later
AFV_LOCAL void afv_tables_pair_scratch(afv_ctx *c, std::vector<ScratchSeg> &dev, std::vector<ScratchSeg> &pin) {
    std::lock_guard<std::mutex> g(g_reg_mutex);
    for (afv_table *t : g_tables) {
        if (t->c != c || !t->pair_cap) continue;
        const size_t pc = (size_t)t->pair_cap, n_pairs = pc * 2 * sizeof(int32_t), n_out = pc * t->cap * sizeof(int32_t), n_nm = pc * sizeof(int32_t);
        dev.push_back(ScratchSeg{t->d_pairs, n_pairs});
        dev.push_back(ScratchSeg{t->d_out, n_out});
        dev.push_back(ScratchSeg{t->d_nm, n_nm});
        pin.push_back(ScratchSeg{t->h_pin, n_pairs + n_nm + n_out});  // [2][pair_cap] pairs, [pair_cap] counts, [pair_cap][cap] matches
    }
}

static int check_pairs(const afv_table *t, const int32_t *pa, const int32_t *pb, int npairs) {
    for (int i = 0; i < npairs; ++i)
        if (pa[i] < 0 || pa[i] >= t->nsets || pb[i] < 0 || pb[i] >= t->nsets) return AFV_EINVAL;
    return AFV_OK;
}

extern "C" int afv_table_match_pairs_device(afv_table *t, const int32_t *d_pair_a, const int32_t *d_pair_b, int npairs, float th_low,
                                            float nnratio, int check_orientation, int32_t *d_match12, int32_t *d_nmatches, void *stream) {
    if (!t || !d_pair_a || !d_pair_b || npairs < 1 || !d_match12 || !d_nmatches) return AFV_EINVAL;
    afv_ctx *c = t->c;
    HIPCHK(c, hipSetDevice(c->device));
    if (t->float_dim)
        return afv_match_l2_pairs_core(c, reinterpret_cast<const float *>(t->d_desc), check_orientation ? t->d_angle : nullptr, t->d_n, t->cap,
                                       t->float_dim, d_pair_a, d_pair_b, npairs, th_low, nnratio, d_match12, d_nmatches,
                                       stream ? (hipStream_t)stream : c->stream);
    return afv_match_pairs_core(c, t->d_desc, t->d_angle, 1, t->d_n, t->cap, d_pair_a, d_pair_b, npairs, th_low, nnratio,
                                check_orientation, d_match12, d_nmatches, stream ? (hipStream_t)stream : c->stream, t->words);
}

extern "C" int afv_table_match_pairs(afv_table *t, const int32_t *pair_a, const int32_t *pair_b, int npairs, float th_low, float nnratio,
                                     int check_orientation, int32_t *match12, int32_t *nmatches) {
    if (!t || !pair_a || !pair_b || npairs < 1 || !nmatches) return AFV_EINVAL;
    if (check_pairs(t, pair_a, pair_b, npairs)) return AFV_EINVAL;
    afv_ctx *c = t->c;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = table_reserve_pairs(t, npairs);
    if (rc) return rc;
    int32_t *hp = t->h_pin, *h_nm = hp + 2 * (size_t)t->pair_cap, *h_out = h_nm + t->pair_cap;
    std::memcpy(hp, pair_a, (size_t)npairs * sizeof(int32_t));
    std::memcpy(hp + t->pair_cap, pair_b, (size_t)npairs * sizeof(int32_t));
    HIPCHK(c, hipMemcpyAsync(t->d_pairs, hp, (size_t)t->pair_cap * 2 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (t->float_dim)
        rc = afv_match_l2_pairs_core(c, reinterpret_cast<const float *>(t->d_desc), check_orientation ? t->d_angle : nullptr, t->d_n, t->cap,
                                     t->float_dim, t->d_pairs, t->d_pairs + t->pair_cap, npairs, th_low, nnratio, t->d_out, t->d_nm, c->stream);
    else
        rc = afv_match_pairs_core(c, t->d_desc, t->d_angle, 1, t->d_n, t->cap, t->d_pairs, t->d_pairs + t->pair_cap, npairs, th_low, nnratio,
                                  check_orientation, t->d_out, t->d_nm, c->stream, t->words);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(h_nm, t->d_nm, (size_t)npairs * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (match12)
        HIPCHK(c, hipMemcpyAsync(h_out, t->d_out, (size_t)npairs * t->cap * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(nmatches, h_nm, (size_t)npairs * sizeof(int32_t));
    if (match12) std::memcpy(match12, h_out, (size_t)npairs * t->cap * sizeof(int32_t));
    return afv_check_resolve_guard(c, nmatches, npairs);
}

// ---- BoW-guided / triangulation batches over the table: the kernels of k_match.hip with job records that point into
// the table; per call only the merge-joined segment lists (host work, FeatureMatcher.cc:205-276) are uploaded.  The routes below check
// their arguments and describe the sides; afv_match_jobs.hip stages and launches ----
// a slot as one side of a job: everything but the FeatureVector's node structure is on the device
AFV_LOCAL MatchSide table_side(const afv_table *t, int slot) {
    const size_t row0 = (size_t)slot * t->cap, plane = (size_t)t->nsets * t->cap;
    const HostFeatVec &fv = t->fv[slot];
    MatchSide s;
    s.on_device = s.valid_on_device = true;
    s.n = t->h_n[slot];
    s.desc_bytes = t->desc_bytes, s.words = t->words, s.fdim = t->float_dim;
    s.rows = t->d_desc + row0 * table_pitch(t);
    s.idx = t->d_idx + row0;
    s.idx_host = fv.seg_idx.data();
    s.valid = t->d_valid ? t->d_valid + row0 : nullptr;  // FeatureMatcher.cc:593-597 / :609-613, :216-222
    s.angle = t->d_angle + row0;
    s.node_id = fv.node_id.data(), s.seg_ptr = fv.seg_ptr.data(), s.nnodes = (int)fv.node_id.size();
    if (t->d_geo) {
        s.x = t->d_geo + row0, s.y = t->d_geo + plane + row0, s.sigma2 = t->d_geo + 2 * plane + row0;
        s.u_right = t->d_geo + 3 * plane + row0;  // -1 everywhere for a monocular keyframe (afv_table_set_geometry)
    }
    return s;
}

// "no shared node" must not be confused with "FeatureVector never stored" (or, for triangulation, geometry never stored)
AFV_LOCAL int check_slot_ready(const afv_table *t, int s, bool need_geo, const char *who) {
    if (t->h_n[s] > 0 && (!t->has_fv[s] || (need_geo && !t->has_geo[s]))) {
        t->c->last_error = std::string(who) + ": set " + std::to_string(s) + (need_geo ? " lacks its FeatureVector or geometry"
                                                                                        : " holds features but no FeatureVector (afv_table_set_featvec)");
        return AFV_EINVAL;
    }
    return AFV_OK;
}

static int table_match_bow_impl(afv_table *t, const int32_t *pair_a, const int32_t *pair_b, int npairs, float th_low, float nnratio,
                                int check_orientation, int32_t *match12, int32_t *nmatches) {
    if (!t->d_idx) return AFV_EINVAL;  // no FeatureVector was ever stored
    MatchBatch B;
    B.per_node = true;
    B.out_stride = t->cap;
    for (int p = 0; p < npairs; ++p) {
        for (int s : {pair_a[p], pair_b[p]}) {
            if (check_slot_ready(t, s, false, "afv_table_match_bow")) return AFV_EINVAL;
            B.sides.push_back(table_side(t, s));
        }
        B.jobs.push_back(MatchJobSpec{2 * p, 2 * p + 1, th_low, nnratio, check_orientation, AFV_MATCH_KF_KF});
    }
    return afv_match_jobs_run(t->c, B, match12, nmatches);
}

extern "C" int afv_table_match_bow(afv_table *t, const int32_t *pair_a, const int32_t *pair_b, int npairs, float th_low, float nnratio,
                                   int check_orientation, int32_t *match12, int32_t *nmatches) {
    if (!t || !pair_a || !pair_b || npairs < 1 || !nmatches) return AFV_EINVAL;
    if (check_pairs(t, pair_a, pair_b, npairs)) return AFV_EINVAL;
    return guarded(t->c, [&] { return table_match_bow_impl(t, pair_a, pair_b, npairs, th_low, nnratio, check_orientation, match12, nmatches); });
}

// Relocalisation batch: SearchByBoW(KF, Frame) (FeatureMatcher.cc:186-283) of ONE frame against `nslots` candidate keyframes of the
// table (Tracking::Relocalization, Tracking.cc:1162,1182: a loop over the candidates of DetectRelocalizationCandidates).  The frame
// travels once (descriptors, angles, FeatureVector feature indices); per candidate only the merge-join of the two FeatureVectors (host,
// a few hundred ints).  M3 rules: validity on the keyframe side only (:216-222), a frame feature that already has a match is skipped
// (:232), accept best <= TH_LOW (:250), rotation histogram keyed by the frame feature (:259).
// `fr` != null: the frame side is a resident afv_frame (descriptors, angles and the FeatureVector body are on the device already; its node
// structure on the host side of the handle) and F only carries n
static int table_match_bow_frame_impl(afv_table *t, const int32_t *slots, int nslots, const afv_frame_view *F, float th_low, float nnratio,
                                      int check_orientation, int32_t *match_f, int32_t *nmatches, const afv_frame *fr = nullptr) {
    if (!t->d_idx) return AFV_EINVAL;  // no FeatureVector was ever stored
    MatchBatch B;
    B.per_node = true;
    B.out_stride = std::max(F->n, 1);
    for (int p = 0; p < nslots; ++p) {
        const int s = slots[p];
        if (s < 0 || s >= t->nsets) return AFV_EINVAL;
        if (check_slot_ready(t, s, false, "afv_table_match_bow_frame")) return AFV_EINVAL;
        B.sides.push_back(table_side(t, s));
        B.jobs.push_back(MatchJobSpec{p, nslots, th_low, nnratio, check_orientation, AFV_MATCH_KF_FRAME});
    }
    MatchSide f;  // the frame: one side of every job, it travels once; no validity on the frame side (FeatureMatcher.cc:216-222)
    f.n = F->n;
    f.desc_bytes = t->desc_bytes, f.words = t->words, f.fdim = t->float_dim;
    if (fr) {
        f.on_device = true;
        f.rows = fr->d_desc, f.idx = fr->d_seg_idx, f.angle = fr->d_angle;
        f.node_id = fr->fv_node_id.data(), f.seg_ptr = fr->fv_seg_ptr.data(), f.nnodes = (int)fr->fv_node_id.size();
    } else {  // the view's rows are packed at the table's width; the runner pads them to its pitch
        if (afv_featvec_check(F->node_id, F->seg_ptr, F->seg_idx, F->nnodes, F->n)) return AFV_EINVAL;
        f.rows = F->desc32, f.angle = check_orientation ? F->angle : nullptr;
        if (F->nnodes > 0) f.node_id = F->node_id, f.seg_ptr = F->seg_ptr, f.idx = F->seg_idx, f.nnodes = F->nnodes;
    }
    B.sides.push_back(f);
    return afv_match_jobs_run(t->c, B, F->n ? match_f : nullptr, nmatches);
}

extern "C" int afv_table_match_bow_frame(afv_table *t, const int32_t *slots, int nslots, const afv_frame_view *frame, float th_low,
                                         float nnratio, int check_orientation, int32_t *match_f, int32_t *nmatches) {
    if (!t || !slots || nslots < 1 || !frame || !nmatches) return AFV_EINVAL;
    if (frame->n < 0 || frame->n > AFV_MAX_SIDE || (frame->n > 0 && !frame->desc32) || frame->nnodes < 0) return AFV_EINVAL;
    if (frame->nnodes > 0 && (!frame->node_id || !frame->seg_ptr || !frame->seg_idx)) return AFV_EINVAL;
    if (check_orientation && frame->n > 0 && !frame->angle) return AFV_EINVAL;
    return guarded(t->c, [&] { return table_match_bow_frame_impl(t, slots, nslots, frame, th_low, nnratio, check_orientation, match_f, nmatches); });
}

extern "C" int afv_table_match_bow_frame_h(afv_table *t, const int32_t *slots, int nslots, afv_frame *f, float th_low, float nnratio,
                                           int check_orientation, int32_t *match_f, int32_t *nmatches) {
    if (!t || !slots || nslots < 1 || !f || !nmatches) return AFV_EINVAL;
    if (f->c != t->c || !f->has_features || !f->has_fv) return AFV_EINVAL;  // afv_frame_bow_transform first
    if (f->float_dim != t->float_dim || f->desc_bytes != t->desc_bytes) return AFV_EUNSUPPORTED;  // rows of the table's kind and width / float dimension only
    afv_frame_view view{};
    view.n = f->n;
    return guarded(t->c, [&] { return table_match_bow_frame_impl(t, slots, nslots, &view, th_low, nnratio, check_orientation, match_f, nmatches, f); });
}

// Words in common and Vocabulary::score of nq query BowVectors against the slots: ONE launch of k_score_bow over (slot groups, queries).
// What travels: the query records (host-array queries with their entries), one state byte per slot; the results come back [nq][nsets].
static int table_score_bow_impl(afv_table *t, const afv_bow_query *caller_q, int nq, const uint8_t *slot_mask, int32_t *common, double *score,
                                int32_t *first_common) {
    afv_ctx *c = t->c;
    std::vector<afv_bow_query> q;
    if (!afv_load_jobs(caller_q, nq, sizeof(afv_bow_query), q)) return AFV_EINVAL;
    const int nsets = t->nsets, cap = t->cap;
    // which slots are scored: 1 = holds features and a BowVector
    std::vector<uint8_t> state((size_t)nsets, 0);
    for (int s = 0; s < nsets; ++s) {
        if (slot_mask && !slot_mask[s]) continue;
        if (t->h_n[s] <= 0) continue;
        if (!t->has_bow[s]) {
            if (!slot_mask) continue;  // a sweep reports the slot as absent; naming it is an error
            c->last_error = "afv_table_score_bow: set " + std::to_string(s) + " holds features but no BowVector (afv_table_set_bowvec)";
            return AFV_EINVAL;
        }
        state[(size_t)s] = 1;
    }
    HIPCHK(c, hipSetDevice(c->device));
    Blob b(c);
    std::vector<DevBowQuery> dq((size_t)nq);
    std::vector<size_t> host_word_off((size_t)nq, 0), host_val_off((size_t)nq, 0);
    for (int i = 0; i < nq; ++i) {
        const afv_bow_query &Q = q[(size_t)i];
        DevBowQuery &D = dq[(size_t)i];
        D = DevBowQuery{nullptr, nullptr, 0, 0};
        if (Q.kind == AFV_BOW_QUERY_SLOT) {
            if (Q.slot < 0 || Q.slot >= nsets || !t->has_bow[Q.slot]) {
                c->last_error = "afv_table_score_bow: query slot " + std::to_string(Q.slot) + " has no BowVector";
                return AFV_EINVAL;
            }
            D.word = t->d_bow_word + (size_t)Q.slot * cap;
            D.value = t->d_bow_value + (size_t)Q.slot * cap;
            D.n = t->h_bow_n[Q.slot];
        } else if (Q.kind == AFV_BOW_QUERY_FRAME) {
            if (!Q.frame || Q.frame->c != c || !Q.frame->has_bow) return AFV_EINVAL;  // afv_frame_bow_transform on a vocabulary with weights first
            D.word = Q.frame->d_bow_word;
            D.value = Q.frame->d_bow_value;
            D.n = Q.frame->bow_n;
        } else if (Q.kind == AFV_BOW_QUERY_HOST) {
            if (Q.n < 0 || Q.n > AFV_BOW_MAX_ENTRIES || (Q.n > 0 && (!Q.word || !Q.value))) return AFV_EINVAL;
            for (int k = 0; k < Q.n; ++k)
                if (Q.word[k] < 0 || (k > 0 && Q.word[k] <= Q.word[k - 1])) return AFV_EINVAL;
            host_word_off[(size_t)i] = b.put(Q.word, (size_t)Q.n * sizeof(int32_t));
            host_val_off[(size_t)i] = b.put(Q.value, (size_t)Q.n * sizeof(double));
            D.n = Q.n;
        } else {
            return AFV_EINVAL;
        }
    }
    const bool any_scored = std::find(state.begin(), state.end(), (uint8_t)1) != state.end();
    if (any_scored && !t->d_bow_word) return AFV_EINVAL;
    const size_t state_off = b.put(state.data(), (size_t)nsets);
    const size_t q_off = b.reserve((size_t)nq * sizeof(DevBowQuery));
    const size_t in_bytes = b.h.size();
    const size_t cells = (size_t)nq * nsets;
    const size_t score_off = b.reserve_scratch(cells * sizeof(double)), common_off = b.reserve_scratch(cells * sizeof(int32_t));
    const size_t first_off = first_common ? b.reserve_scratch(cells * sizeof(int32_t)) : 0;
    const int rc = ensure_match_buffer(c, b.h.size());
    if (rc) return rc;
    for (int i = 0; i < nq; ++i)
        if (q[(size_t)i].kind == AFV_BOW_QUERY_HOST) {
            dq[(size_t)i].word = reinterpret_cast<const int32_t *>(c->d_match + host_word_off[(size_t)i]);
            dq[(size_t)i].value = reinterpret_cast<const double *>(c->d_match + host_val_off[(size_t)i]);
        }
    std::memcpy(b.h.data() + q_off, dq.data(), (size_t)nq * sizeof(DevBowQuery));
    HIPCHK(c, hipMemcpyAsync(c->d_match, b.h.data(), in_bytes, hipMemcpyHostToDevice, c->stream));
    afv_launch_score_bow(reinterpret_cast<const DevBowQuery *>(c->d_match + q_off), nq, t->d_bow_word, t->d_bow_value, t->d_bow_n,
                         c->d_match + state_off, nsets, cap, reinterpret_cast<int32_t *>(c->d_match + common_off),
                         reinterpret_cast<double *>(c->d_match + score_off),
                         first_common ? reinterpret_cast<int32_t *>(c->d_match + first_off) : nullptr, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, b.fetch(common, common_off, cells * sizeof(int32_t), c->stream));
    HIPCHK(c, b.fetch(score, score_off, cells * sizeof(double), c->stream));
    if (first_common) HIPCHK(c, b.fetch(first_common, first_off, cells * sizeof(int32_t), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    b.finish();
    return AFV_OK;
}

extern "C" int afv_table_score_bow(afv_table *t, const afv_bow_query *q, int nq, const uint8_t *slot_mask, int32_t *common, double *score,
                                   int32_t *first_common) {
    if (!t || !q || nq < 1 || nq > 65535 || !common || !score) return AFV_EINVAL;
    return guarded(t->c, [&] { return table_score_bow_impl(t, q, nq, slot_mask, common, score, first_common); });
}

// KeyFrame::KeyFrame(Frame &F, ...) (src/KeyFrame.cc:36-60) on the device: one kernel copies the frame's arrays into the slot's rows of the
// table planes; the FeatureVector's node structure goes host to host
extern "C" int afv_table_set_from_frame(afv_table *t, int slot, afv_frame *f) {
    if (!t || !f || slot < 0 || slot >= t->nsets || f->c != t->c || !f->has_features) return AFV_EINVAL;
    if (f->float_dim != t->float_dim || f->desc_bytes != t->desc_bytes) return AFV_EUNSUPPORTED;  // rows of the table's kind and width / float dimension only
    if (f->n > t->cap) return AFV_ECAPACITY;
    afv_ctx *c = t->c;
    return guarded(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        const size_t plane = (size_t)t->nsets * t->cap;
        if (!t->d_geo) {  // a promoted frame brings its geometry: the planes exist from the first promotion on
            HIPCHK(c, hipMalloc(&t->d_geo, 4 * plane * sizeof(float)));
        }
        if (!t->d_scale) HIPCHK(c, hipMalloc(&t->d_scale, 4 * plane * sizeof(float)));  // ... and its sizes, depths and keypoints
        if (f->has_fv && !t->d_idx) HIPCHK(c, hipMalloc(&t->d_idx, plane * sizeof(int32_t)));
        PromoteArgs A{};
        A.f_desc = reinterpret_cast<const uint4 *>(f->d_desc);
        A.f_angle = f->d_angle; A.f_x = f->d_x; A.f_y = f->d_y; A.f_sigma2 = f->d_sigma2; A.f_ur = f->d_ur;
        A.f_seg_idx = f->has_fv ? f->d_seg_idx : nullptr;
        A.t_desc = reinterpret_cast<uint4 *>(t->d_desc + (size_t)slot * t->cap * table_pitch(t));  // the frame's rows have the same pitch
        A.t_angle = t->d_angle + (size_t)slot * t->cap;
        A.t_x = t->d_geo + (size_t)slot * t->cap;
        A.t_y = t->d_geo + plane + (size_t)slot * t->cap;
        A.t_sigma2 = t->d_geo + 2 * plane + (size_t)slot * t->cap;
        A.t_ur = t->d_geo + 3 * plane + (size_t)slot * t->cap;
        A.f_size = f->d_size; A.f_depth = f->has_depth ? f->d_depth : nullptr; A.f_kps = f->d_kps;
        A.t_size = t->d_scale + (size_t)slot * t->cap;
        A.t_depth = t->d_scale + plane + (size_t)slot * t->cap;
        A.t_xd = t->d_scale + 2 * plane + (size_t)slot * t->cap;
        A.t_yd = t->d_scale + 3 * plane + (size_t)slot * t->cap;
        A.t_idx = (f->has_fv && t->d_idx) ? t->d_idx + (size_t)slot * t->cap : nullptr;
        A.t_valid = t->d_valid ? t->d_valid + (size_t)slot * t->cap : nullptr;
        A.t_n = t->d_n + slot;
        A.n = f->n; A.cap = t->cap; A.nkept = f->has_fv ? f->fv_total : 0;
        afv_launch_table_promote(&A, f->n, t->cap, t->words, c->stream);
        HIPCHK(c, hipGetLastError());
        t->h_n[slot] = f->n;
        t->fv[slot] = HostFeatVec();
        t->has_fv[slot] = 0;
        if (f->has_fv) {
            t->fv[slot].node_id = f->fv_node_id;
            t->fv[slot].seg_ptr = f->fv_seg_ptr;
            // the body lives on the device only; the host copy is fetched on demand by the few paths that read it (triangulation row map)
            t->fv[slot].seg_idx.clear();
            t->fv_body_on_device[slot] = 1;
            t->has_fv[slot] = 1;
        }
        t->has_geo[slot] = 1;
        t->has_scale[slot] = 1;
        afv_kffuse_slot_reset(t, slot);  // a new keyframe: the pose and the mvpMapPoints of the slot's previous occupant are not its own
        // ... and its keyPtsInf, the information plane (what PoseOptimization reads on the frame, OptimizeSim3 on the keyframe)
        if (!t->d_inf) HIPCHK(c, hipMalloc(&t->d_inf, plane * sizeof(float)));
        if (f->n) HIPCHK(c, hipMemcpyAsync(t->d_inf + (size_t)slot * t->cap, f->d_inf, (size_t)f->n * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        t->has_inf[slot] = 1;
        // the BowVector comes along like the FeatureVector (a frame without one leaves the slot without one)
        t->has_bow[slot] = 0;
        t->h_bow_n[slot] = 0;
        if (f->has_bow) {
            const int rcb = table_ensure_bow(t);
            if (rcb) return rcb;
            if (f->bow_n > t->cap) return AFV_ECAPACITY;
            if (f->bow_n) {
                HIPCHK(c, hipMemcpyAsync(t->d_bow_word + (size_t)slot * t->cap, f->d_bow_word, (size_t)f->bow_n * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
                HIPCHK(c, hipMemcpyAsync(t->d_bow_value + (size_t)slot * t->cap, f->d_bow_value, (size_t)f->bow_n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
            }
            HIPCHK(c, hipMemcpyAsync(t->d_bow_n + slot, f->d_bow_n, sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
            t->h_bow_n[slot] = f->bow_n;
            t->has_bow[slot] = 1;
        } else if (t->d_bow_n) {
            HIPCHK(c, hipMemsetAsync(t->d_bow_n + slot, 0, sizeof(int32_t), c->stream));
        }
        return AFV_OK;
    });
}

// host copy of a slot's FeatureVector body when it was promoted from a frame (device to device): fetched once, on first need
AFV_LOCAL int table_fetch_fv_body(afv_table *t, int slot) {
    if (!t->fv_body_on_device[slot]) return AFV_OK;
    afv_ctx *c = t->c;
    HostFeatVec &f = t->fv[slot];
    const int total = f.seg_ptr.empty() ? 0 : f.seg_ptr.back();
    f.seg_idx.assign((size_t)total, 0);
    if (total) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(f.seg_idx.data(), t->d_idx + (size_t)slot * t->cap, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    t->fv_body_on_device[slot] = 0;
    return AFV_OK;
}

static int table_match_tri_impl(afv_table *t, const int32_t *pair_a, const int32_t *pair_b, const afv_table_tri_job *caller_geo, int npairs,
                                int32_t *match12, int32_t *nmatches) {
    std::vector<afv_table_tri_job> geo;
    if (!afv_load_jobs(caller_geo, npairs, offsetof(afv_table_tri_job, only_stereo), geo)) return AFV_EINVAL;
    for (int p = 0; p < npairs; ++p) {
        if (geo[p].only_stereo != 0 && geo[p].only_stereo != 1) return AFV_EINVAL;
        const int rcf = table_fetch_fv_body(t, pair_a[p]);  // the row map of side a reads the body on the host
        if (rcf) return rcf;
    }
    if (!t->d_idx || !t->d_geo) return AFV_EINVAL;
    MatchBatch B;
    B.tri = true;
    B.out_stride = t->cap;
    for (int p = 0; p < npairs; ++p) {
        const uint8_t *has_mp[2] = {geo[p].has_mp1, geo[p].has_mp2};
        for (int k = 0; k < 2; ++k) {
            const int s = k ? pair_b[p] : pair_a[p];
            if (check_slot_ready(t, s, true, "afv_table_match_triangulation")) return AFV_EINVAL;
            MatchSide m = table_side(t, s);
            m.valid = m.n ? has_mp[k] : nullptr;  // host masks "already has a map point" instead of the table's validity plane
            m.valid_on_device = false;
            B.sides.push_back(m);
        }
        B.jobs.push_back(MatchJobSpec{2 * p, 2 * p + 1, geo[p].th_low, 0.f, 0, AFV_MATCH_KF_KF, geo[p].F12, geo[p].ex, geo[p].ey, geo[p].only_stereo});
    }
    return afv_match_jobs_run(t->c, B, match12, nmatches);
}

extern "C" int afv_table_match_triangulation(afv_table *t, const int32_t *pair_a, const int32_t *pair_b, const afv_table_tri_job *geo,
                                             int npairs, int32_t *match12, int32_t *nmatches) {
    if (!t || !pair_a || !pair_b || !geo || npairs < 1 || !match12 || !nmatches) return AFV_EINVAL;
    if (check_pairs(t, pair_a, pair_b, npairs)) return AFV_EINVAL;
    return guarded(t->c, [&] { return table_match_tri_impl(t, pair_a, pair_b, geo, npairs, match12, nmatches); });
}

// ------------------------------------------------------------------------------------------------------------------
// RCCL, resolved at run time
// ------------------------------------------------------------------------------------------------------------------
namespace {
struct RcclApi {
    void *handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*Broadcast)(const void *, void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    bool ok = false;
};

const RcclApi &rccl() {
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        // 1. a copy some other component (PyTorch) already mapped; 2. the system RCCL
        const char *names[] = {"librccl.so.1", "librccl.so"};
        for (const char *n : names)
            if (!api.handle) api.handle = dlopen(n, RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL);
        const char *paths[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char *n : paths)
            if (!api.handle) api.handle = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (!api.handle) return;
#define AFV_SYM(field, name) api.field = reinterpret_cast<decltype(api.field)>(dlsym(api.handle, name))
        AFV_SYM(GetUniqueId, "ncclGetUniqueId");
        AFV_SYM(CommInitRank, "ncclCommInitRank");
        AFV_SYM(CommDestroy, "ncclCommDestroy");
        AFV_SYM(Broadcast, "ncclBroadcast");
        AFV_SYM(AllGather, "ncclAllGather");
        AFV_SYM(GetErrorString, "ncclGetErrorString");
#undef AFV_SYM
        api.ok = api.GetUniqueId && api.CommInitRank && api.CommDestroy && api.Broadcast && api.AllGather;
    });
    return api;
}
}  // namespace

#define NCCLCHK(ctx, call)                                                                                  \
    do {                                                                                                    \
        ncclResult_t r_ = (call);                                                                           \
        if (r_ != ncclSuccess) {                                                                            \
            (ctx)->last_error = std::string(#call) + ": " + (rccl().GetErrorString ? rccl().GetErrorString(r_) : "RCCL error"); \
            return AFV_EHIP;                                                                                \
        }                                                                                                   \
    } while (0)

extern "C" int afv_comm_unique_id(uint8_t id[AFV_COMM_ID_BYTES]) {
    static_assert(AFV_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "id size");
    if (!id) return AFV_EINVAL;
    if (!rccl().ok) return AFV_EUNSUPPORTED;
    ncclUniqueId u;
    if (rccl().GetUniqueId(&u) != ncclSuccess) return AFV_EHIP;
    std::memcpy(id, u.internal, AFV_COMM_ID_BYTES);
    return AFV_OK;
}

extern "C" int afv_comm_create(afv_ctx *c, const uint8_t id[AFV_COMM_ID_BYTES], int nranks, int rank, afv_comm **out) {
    if (!c || !id || !out || nranks < 1 || rank < 0 || rank >= nranks) return AFV_EINVAL;
    *out = nullptr;
    if (!rccl().ok) {
        c->last_error = "RCCL (librccl.so.1) not found";
        return AFV_EUNSUPPORTED;
    }
    HIPCHK(c, hipSetDevice(c->device));
    afv_comm *m = new (std::nothrow) afv_comm();
    if (!m) return AFV_ENOMEM;
    m->c = c;
    m->nranks = nranks;
    m->rank = rank;
    ncclUniqueId u;
    std::memcpy(u.internal, id, AFV_COMM_ID_BYTES);
    const ncclResult_t r = rccl().CommInitRank(&m->comm, nranks, u, rank);
    if (r != ncclSuccess) {
        c->last_error = std::string("ncclCommInitRank: ") + (rccl().GetErrorString ? rccl().GetErrorString(r) : "RCCL error");
        delete m;
        return AFV_EHIP;
    }
    try {
        std::lock_guard<std::mutex> g(g_reg_mutex);
        g_comms.push_back(m);
    } catch (...) {
        (void)rccl().CommDestroy(m->comm);
        delete m;
        return AFV_ENOMEM;
    }
    *out = m;
    return AFV_OK;
}

extern "C" void afv_comm_destroy(afv_comm *m) {
    if (!m) return;
    {
        std::lock_guard<std::mutex> g(g_reg_mutex);
        auto it = std::find(g_comms.begin(), g_comms.end(), m);
        if (it == g_comms.end()) return;
        g_comms.erase(it);
    }
    if (m->c) {
        (void)hipSetDevice(m->c->device);
        (void)hipStreamSynchronize(m->c->stream);
    }
    if (m->comm) (void)rccl().CommDestroy(m->comm);
    delete m;
}

extern "C" int afv_comm_rank(const afv_comm *m) { return m ? m->rank : AFV_EINVAL; }
extern "C" int afv_comm_size(const afv_comm *m) { return m ? m->nranks : AFV_EINVAL; }

extern "C" int afv_comm_broadcast(afv_comm *m, void *d_buf, size_t bytes, int root, void *stream) {
    if (!m || (!d_buf && bytes) || root < 0 || root >= m->nranks) return AFV_EINVAL;
    if (!bytes) return AFV_OK;
    afv_ctx *c = m->c;
    HIPCHK(c, hipSetDevice(c->device));
    NCCLCHK(c, rccl().Broadcast(d_buf, d_buf, bytes, ncclUint8, root, m->comm, stream ? (hipStream_t)stream : c->stream));
    return AFV_OK;
}

extern "C" int afv_comm_allgather(afv_comm *m, const void *d_send, void *d_recv, size_t bytes_per_rank, void *stream) {
    if (!m || !d_send || !d_recv) return AFV_EINVAL;
    if (!bytes_per_rank) return AFV_OK;
    afv_ctx *c = m->c;
    HIPCHK(c, hipSetDevice(c->device));
    NCCLCHK(c, rccl().AllGather(d_send, d_recv, bytes_per_rank, ncclUint8, m->comm, stream ? (hipStream_t)stream : c->stream));
    return AFV_OK;
}

extern "C" int afv_table_broadcast(afv_comm *m, afv_table *t, int root, float *elapsed_ms) {
    if (!m || !t || m->c != t->c || root < 0 || root >= m->nranks) return AFV_EINVAL;
    afv_ctx *c = t->c;
    return guarded(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        // what the root holds: optional planes (ranks allocate them on demand so the buffers exist everywhere) and the length of its
        // replica image (host-side FeatureVector structure + per-set flags)
        std::vector<int32_t> blob;
        if (m->rank == root) table_pack_meta(t, blob);
        // ... and its shape: every rank compares it with its own table and ALL ranks learn every verdict (one all-gather of a flag) before any
        // plane moves, so that a table of another shape or row width on any rank is refused everywhere instead of mismatching the
        // lengths of the broadcasts below
        // (the kind travels next to the width: 64-byte binary rows and rows of 16 floats have the same pitch and the same byte size)
        int32_t flags[9] = {t->d_idx != nullptr, (t->d_geo != nullptr) | ((t->d_scale != nullptr) << 1) | ((t->d_inf != nullptr) << 2) /* bit 1: the scale planes, bit 2: the information plane */, t->d_valid != nullptr, (int32_t)blob.size(), t->nsets, t->cap, t->desc_bytes, t->float_dim,
                            t->d_bow_word != nullptr};
        int32_t *d_flags = nullptr;
        HIPCHK(c, hipMalloc(&d_flags, sizeof(flags) + (size_t)(m->nranks + 1) * sizeof(int32_t)));
        int32_t *d_ok = d_flags + 9, *d_oks = d_ok + 1;
        hipError_t e = hipMemcpyAsync(d_flags, flags, sizeof(flags), hipMemcpyHostToDevice, c->stream);
        int rc = e == hipSuccess ? afv_comm_broadcast(m, d_flags, sizeof(flags), root, c->stream) : AFV_EHIP;
        if (rc == AFV_OK) e = hipMemcpyAsync(flags, d_flags, sizeof(flags), hipMemcpyDeviceToHost, c->stream);
        if (rc == AFV_OK && e == hipSuccess) e = hipStreamSynchronize(c->stream);
        std::vector<int32_t> oks((size_t)m->nranks, 0);
        if (rc == AFV_OK && e == hipSuccess) {
            // 1: the root's shape; 2: its nsets and cap, but another kind or float dimension; 0: any other difference
            const int32_t ok = !(flags[4] == t->nsets && flags[5] == t->cap) ? 0 : (flags[7] != t->float_dim ? 2 : flags[6] == t->desc_bytes);
            e = hipMemcpyAsync(d_ok, &ok, sizeof(ok), hipMemcpyHostToDevice, c->stream);
            if (e == hipSuccess) rc = afv_comm_allgather(m, d_ok, d_oks, sizeof(int32_t), c->stream);
            if (rc == AFV_OK && e == hipSuccess) e = hipMemcpyAsync(oks.data(), d_oks, oks.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
            if (rc == AFV_OK && e == hipSuccess) e = hipStreamSynchronize(c->stream);
        }
        (void)hipFree(d_flags);
        if (rc) return rc;
        HIPCHK(c, e);
        for (int32_t ok : oks)
            if (ok == 2) {
                c->last_error = "afv_table_broadcast: the tables of the ranks differ in kind (binary / float) or float_dim";
                return AFV_EUNSUPPORTED;
            }
        for (int32_t ok : oks)
            if (!ok) {
                c->last_error = "afv_table_broadcast: the tables of the ranks differ in nsets, cap or desc_bytes";
                return AFV_EINVAL;
            }
        if (flags[3] < 1) return AFV_EINVAL;
        const size_t plane = (size_t)t->nsets * t->cap;
        if (flags[0] && !t->d_idx) HIPCHK(c, hipMalloc(&t->d_idx, plane * sizeof(int32_t)));
        if ((flags[1] & 1) && !t->d_geo) HIPCHK(c, hipMalloc(&t->d_geo, 4 * plane * sizeof(float)));
        if ((flags[1] & 2) && !t->d_scale) HIPCHK(c, hipMalloc(&t->d_scale, 4 * plane * sizeof(float)));
        if ((flags[1] & 4) && !t->d_inf) HIPCHK(c, hipMalloc(&t->d_inf, plane * sizeof(float)));
        if (flags[2] && !t->d_valid) HIPCHK(c, hipMalloc(&t->d_valid, plane));
        if (flags[8]) {
            const int rcb = table_ensure_bow(t);
            if (rcb) return rcb;
        }
        int32_t *d_meta = nullptr;
        HIPCHK(c, hipMalloc(&d_meta, (size_t)flags[3] * sizeof(int32_t)));
        struct Free { void *p; ~Free() { (void)hipFree(p); } } free_meta{d_meta};
        if (m->rank == root) HIPCHK(c, hipMemcpyAsync(d_meta, blob.data(), blob.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipEventRecord(t->ev0, c->stream));
        rc = afv_comm_broadcast(m, t->d_desc, plane * table_pitch(t), root, c->stream);
        if (!rc) rc = afv_comm_broadcast(m, t->d_angle, plane * sizeof(float), root, c->stream);
        if (!rc) rc = afv_comm_broadcast(m, t->d_n, (size_t)t->nsets * sizeof(int32_t), root, c->stream);
        if (!rc && flags[0]) rc = afv_comm_broadcast(m, t->d_idx, plane * sizeof(int32_t), root, c->stream);
        if (!rc && (flags[1] & 1)) rc = afv_comm_broadcast(m, t->d_geo, 4 * plane * sizeof(float), root, c->stream);
        if (!rc && (flags[1] & 2)) rc = afv_comm_broadcast(m, t->d_scale, 4 * plane * sizeof(float), root, c->stream);
        if (!rc && (flags[1] & 4)) rc = afv_comm_broadcast(m, t->d_inf, plane * sizeof(float), root, c->stream);
        if (!rc && flags[2]) rc = afv_comm_broadcast(m, t->d_valid, plane, root, c->stream);
        if (!rc && flags[8]) rc = afv_comm_broadcast(m, t->d_bow_word, plane * sizeof(int32_t), root, c->stream);
        if (!rc && flags[8]) rc = afv_comm_broadcast(m, t->d_bow_value, plane * sizeof(double), root, c->stream);
        if (!rc && flags[8]) rc = afv_comm_broadcast(m, t->d_bow_n, (size_t)t->nsets * sizeof(int32_t), root, c->stream);
        if (!rc) rc = afv_comm_broadcast(m, d_meta, (size_t)flags[3] * sizeof(int32_t), root, c->stream);
        if (rc) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
        HIPCHK(c, hipEventRecord(t->ev1, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (elapsed_ms) HIPCHK(c, hipEventElapsedTime(elapsed_ms, t->ev0, t->ev1));
        if (m->rank == root) {
            rc = afv_table_sync_counts(t);
            return rc ? rc : afv_kffuse_broadcast(m, t, root);
        }
        // receivers: nothing of the previous content survives; counts first, then the FeatureVectors against them
        for (int s = 0; s < t->nsets; ++s) {
            t->fv[s] = HostFeatVec();
            t->has_fv[s] = t->has_geo[s] = t->has_scale[s] = t->has_inf[s] = t->has_bow[s] = 0;
            t->h_bow_n[s] = 0;
        }
        if (!flags[8] && t->d_bow_n) HIPCHK(c, afv_fill(c, t->d_bow_n, 0, (size_t)t->nsets * sizeof(int32_t)));
        if (!flags[2] && t->d_valid) HIPCHK(c, afv_fill(c, t->d_valid, 1, plane));
        rc = afv_table_sync_counts(t);
        if (rc) return rc;
        blob.resize((size_t)flags[3]);
        HIPCHK(c, hipMemcpy(blob.data(), d_meta, blob.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        rc = table_unpack_meta(t, blob.data(), blob.size());
        return rc ? rc : afv_kffuse_broadcast(m, t, root);  // camera, poses and the mvpMapPoints plane (afv_kffuse.hip)
    });
}

extern "C" void afv_shard_range(long n_units, int rank, int nranks, long *lo, long *hi) {
    if (nranks < 1) nranks = 1;
    rank = std::min(std::max(rank, 0), nranks - 1);
    const long base = n_units / nranks, rem = n_units % nranks;
    const long l = rank * base + std::min<long>(rank, rem);
    if (lo) *lo = l;
    if (hi) *hi = l + base + (rank < rem ? 1 : 0);
}

// afv_destroy: whatever the caller forgot to release dies with the context
void afv_table_release_all(afv_ctx *c) {
    std::vector<afv_table *> ts;
    std::vector<afv_comm *> ms;
    {
        std::lock_guard<std::mutex> g(g_reg_mutex);
        for (auto it = g_tables.begin(); it != g_tables.end();)
            if ((*it)->c == c) { ts.push_back(*it); it = g_tables.erase(it); } else ++it;
        for (auto it = g_comms.begin(); it != g_comms.end();)
            if ((*it)->c == c) { ms.push_back(*it); it = g_comms.erase(it); } else ++it;
    }
    for (afv_table *t : ts) table_free(t);
    for (afv_comm *m : ms) {
        if (m->comm && rccl().ok) (void)rccl().CommDestroy(m->comm);
        delete m;
    }
}
