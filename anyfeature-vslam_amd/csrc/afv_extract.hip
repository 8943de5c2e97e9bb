// afv_extract.hip — host runtime of the ORB32 extractor behind the C-ABI of include/afv_hip.h.
// Owns the per-geometry tables of a context (level sizes, resize coefficients, quotas, the one-launch pyramid's plan), stages
// host-pointer calls through one path (stage_images) and enqueues the kernel pipeline
//   resize x (nlevels-1) -> FAST+NMS+Harris -> retainBest x2 + quadtree -> IC + blur + rBRIEF
// for the entry points afv_orb_extract_batch_device / _batch / afv_orb_extract / _detect / _compute and afv_frame_extract.
// Holds no kernel (k_*.hip); the context itself is created and destroyed in afv_api.hip.
#include <chrono>

#include "afv_runtime.h"

// ---- geometry (host).  Mirrors cv::ORB's level sizes / quotas and FeatureExtractor.cpp:97-108 ----
int afv_build_geometry(const afv_orb_params &p, int w, int h, int max_batch, Geo &g) {
    std::memset(&g, 0, sizeof(g));
    if (p.nlevels < 1 || p.nlevels > AFV_MAX_LEVELS || w < 1 || h < 1 || w > 4095 || h > 4095) return AFV_EINVAL;
    g.nlevels = p.nlevels;
    g.width = w;
    g.height = h;
    g.fast_threshold = std::min(std::max(p.fast_threshold, 0), 255);
    {
        const float scale = 1.f / ((1 << 2) * 7 * 255.f);
        g.harris_scale4 = scale * scale * scale * scale;
    }
    g.n_ini = (int)roundf((float)w / (float)h);  // ORBextractor.cc:243
    if (g.n_ini < 1 || g.n_ini > 16) return AFV_EUNSUPPORTED;
    g.h_x = (float)w / (float)g.n_ini;
    // quadtree quotas (FeatureExtractor.cpp:97-108)
    int quota[AFV_MAX_LEVELS], cvq[AFV_MAX_LEVELS];
    afv_level_quotas(p.nfeatures, 1.0f / p.scale_factor, p.nlevels, quota);
    // cv::ORB computeKeyPoints with nfeatures*10 (Feature_orb32.cpp:22), scaleFactor held as double
    afv_level_quotas(p.nfeatures * 10, (float)(1.0 / (double)p.scale_factor), p.nlevels, cvq);
    size_t pyr_off = 0, cand_off = 0;
    int tile_base = 0, sel_base = 0, desc_blk_base = 0;
    for (int l = 0; l < p.nlevels; ++l) {
        LevelGeo &L = g.lv[l];
        L.scale = (float)std::pow((double)p.scale_factor, (double)l);
        L.inv_scale = 1.0f / L.scale;
        L.w = cv_round((float)w * L.inv_scale);
        L.h = cv_round((float)h * L.inv_scale);
        if (L.w < 32 || L.h < 32) return AFV_EUNSUPPORTED;  // single-reflection apron needs >= 32 px levels
        if (l > 0 && !afv_resize_window_ok(g.lv[l - 1].w, g.lv[l - 1].h, L.w, L.h)) return AFV_EUNSUPPORTED;  // level ratio > ~2.37
        L.pitch = (int)align_up((size_t)L.w, 64);
        L.tiles_x = (L.w + FT_W - 1) / FT_W;
        L.tiles_y = (L.h + FT_H - 1) / FT_H;
        L.dv_tiles_x = afv_div_magic((uint32_t)L.tiles_x);
        L.tile_base = tile_base;
        tile_base += L.tiles_x * L.tiles_y;
        L.quota = quota[l];
        L.cv_quota = cvq[l];
        L.cand_cap = ((L.w + 1) / 2) * ((L.h + 1) / 2);
        // DistributeOctTree returns quota .. quota+2 nodes when saturated, but the first split round is unconditional
        // (ORBextractor.cc:283-366) and leaves up to 4 * n_ini nodes even when the quota is smaller
        L.sel_cap = std::max(L.quota + 3, 4 * g.n_ini);
        L.sel_base = sel_base;
        sel_base += L.sel_cap;
        L.desc_blk_base = desc_blk_base;
        desc_blk_base += (L.sel_cap + AFV_KP_PER_BLOCK - 1) / AFV_KP_PER_BLOCK;  // keypoints per k_describe block
        L.pyr_frame_stride = align_up((size_t)L.h * L.pitch + 64, 256);
        L.pyr_off = pyr_off;
        if (l > 0) pyr_off += L.pyr_frame_stride * (size_t)max_batch;
        L.cand_frame_stride = (size_t)L.cand_cap;
        L.cand_off = cand_off;
        cand_off += L.cand_frame_stride * (size_t)max_batch;
    }
    g.total_tiles = tile_base;
    g.dv_total_tiles = afv_div_magic((uint32_t)tile_base);
    g.sel_per_frame = sel_base;
    g.dv_desc_per_frame = afv_div_magic((uint32_t)afv_describe_blocks_per_frame(&g));
    return AFV_OK;
}

size_t afv_geo_pyr_bytes(const Geo &g, int max_batch) {
    const LevelGeo &L = g.lv[g.nlevels - 1];
    return g.nlevels > 1 ? L.pyr_off + L.pyr_frame_stride * (size_t)max_batch : 256;
}
size_t afv_geo_cand_elems(const Geo &g, int max_batch) {
    const LevelGeo &L = g.lv[g.nlevels - 1];
    return L.cand_off + L.cand_frame_stride * (size_t)max_batch;
}

// OpenCV resize_bitExact / interpolation_linear<uchar>::getCoeffs: per destination index {offset, weight of right tap}
static void resize_table(int src, int dst, short2 *t) {
    const double inv_scale = (double)dst / (double)src;
    const double scale = 1.0 / inv_scale;
    for (int d = 0; d < dst; ++d) {
        const double f = scale * ((double)d + 0.5) - 0.5;
        const int i = (int)std::floor(f);
        short2 e;
        if (i >= 0 && src > 1) {
            if (i < src - 1) {
                e.x = (short)i;
                e.y = (short)lrint((f - (double)i) * 256.0);
            } else {
                e.x = (short)(src - 1);
                e.y = 0;
            }
        } else {
            e.x = 0;
            e.y = 0;
        }
        t[d] = e;
    }
}

// Region bookkeeping of k_pyramid_fused (k_pyramid.hip): per level and per tile index of the TOP level, the range a workgroup
// computes (need) and the range it stores (own), x and y separately.  own: the top level is cut into tiles of tw x th; one level
// down a tile owns what lies between the source offsets of its own and of its right / lower neighbour's first pixel (monotone
// tables: a disjoint cover).  need: the owned range (x: widened to whole dwords) united with the source span of the level above.
static int ceil_log2(int v) {
    int lg = 0;
    while ((1 << lg) < v) ++lg;
    return lg;
}
static bool plan_pyr_fuse(const Geo &g, const short2 *tab, const size_t *tab_off_x, const size_t *tab_off_y, int TW, int TH,
                          std::vector<short4> &reg, PyrFusePlan &P) {
    const int NL = g.nlevels, L = NL - 1;
    if (NL < 2 || TW < 4 || (TW & 3) || TH < 1) return false;
    const int ntx = (g.lv[L].w + TW - 1) / TW, nty = (g.lv[L].h + TH - 1) / TH;
    reg.assign((size_t)NL * (ntx + nty), short4{0, 0, 0, 0});
    int maxlen[2][AFV_MAX_LEVELS] = {};
    for (int ax = 0; ax < 2; ++ax) {
        const bool is_x = ax == 0;
        const int nt = is_x ? ntx : nty, T = is_x ? TW : TH;
        auto dim = [&](int l) { return is_x ? g.lv[l].w : g.lv[l].h; };
        auto offs = [&](int l) { return tab + (is_x ? tab_off_x[l] : tab_off_y[l]); };  // table of level l: offsets into level l - 1
        short4 *out = reg.data() + (is_x ? 0 : (size_t)NL * ntx);
        for (int t = 0; t < nt; ++t) {
            int own_lo[AFV_MAX_LEVELS], own_hi[AFV_MAX_LEVELS], lo[AFV_MAX_LEVELS], hi[AFV_MAX_LEVELS];
            own_lo[L] = t * T;
            own_hi[L] = std::min((t + 1) * T, dim(L));
            for (int l = L - 1; l >= 1; --l) {
                own_lo[l] = t == 0 ? 0 : (own_lo[l + 1] < dim(l + 1) ? offs(l + 1)[own_lo[l + 1]].x : dim(l));
                own_hi[l] = t == nt - 1 ? dim(l) : (own_hi[l + 1] < dim(l + 1) ? offs(l + 1)[own_hi[l + 1]].x : dim(l));
            }
            for (int l = L; l >= 1; --l) {
                int a = own_lo[l], b = own_hi[l];
                if (is_x) {
                    a &= ~3;
                    b = (b + 3) & ~3;
                }
                int lo_ = a, hi_ = b - 1;
                if (l < L) {
                    const int n0 = lo[l + 1], n1 = std::min(hi[l + 1], dim(l + 1) - 1);
                    const int lo2 = offs(l + 1)[n0].x, hi2 = std::min(offs(l + 1)[n1].x + 1, dim(l) - 1);
                    if (b > a) {
                        lo_ = std::min(lo_, lo2);
                        hi_ = std::max(hi_, hi2);
                    } else {
                        lo_ = lo2;
                        hi_ = hi2;
                    }
                }
                if (is_x) {
                    lo_ &= ~3;
                    hi_ = lo_ + ((hi_ - lo_ + 4) & ~3) - 1;
                }
                lo[l] = lo_;
                hi[l] = hi_;
                out[(size_t)l * nt + t] = short4{(short)lo_, (short)hi_, (short)own_lo[l], (short)own_hi[l]};
                maxlen[ax][l] = std::max(maxlen[ax][l], hi_ - lo_ + 1);
            }
            {   // the level-0 window
                const int n0 = lo[1], n1 = std::min(hi[1], dim(1) - 1);
                int lo0 = offs(1)[n0].x;
                const int hi0 = std::min(offs(1)[n1].x + 1, dim(0) - 1);
                if (is_x) lo0 &= ~3;
                out[t] = short4{(short)lo0, (short)hi0, 0, 0};
                maxlen[ax][0] = std::max(maxlen[ax][0], hi0 - lo0 + 1);
            }
        }
    }
    std::memset(&P, 0, sizeof(P));
    P.nlevels = NL;
    P.ntx = ntx;
    P.nty = nty;
    for (int l = 0; l < NL; ++l) {
        P.pitch[l] = (int)align_up((size_t)maxlen[0][l], 4);
        P.maxh[l] = maxlen[1][l];
        P.lg_q[l] = ceil_log2(P.pitch[l] / 4);
        if (P.lg_q[l] > 10) return false;  // more dword slots per row than the workgroup has threads
        if (l > 0) {
            P.tabx[l] = (int)tab_off_x[l];
            P.taby[l] = (int)tab_off_y[l];
            // the dword-read form of the level loop: left tap of column c + 3 at most 6 bytes past that of column c
            const short2 *xt = tab + tab_off_x[l];
            bool narrow = true;
            for (int x = 0; x + 3 < g.lv[l].w && narrow; x += 4) narrow = xt[x + 3].x - xt[x].x <= 6;
            P.narrow[l] = narrow ? 1 : 0;
        }
    }
    return true;
}

// the device image of a plan (layout: afv_device.h) and the kernel's arguments / LDS size
static void pack_pyr_fuse(const Geo &g, const short2 *tab, const std::vector<short4> &reg, const PyrFusePlan &P, std::vector<uint8_t> &blob,
                          PyrFuseArgs &A, size_t &lds) {
    const int NL = P.nlevels;
    std::memset(&A, 0, sizeof(A));
    A.nlevels = NL;
    A.ntx = P.ntx;
    A.nty = P.nty;
    A.w0 = g.width;
    PfLevelC C[AFV_MAX_LEVELS];
    std::memset(C, 0, sizeof(C));
    size_t sx = 0, sy = 0;
    for (int l = 0; l < NL; ++l) {
        C[l].lds_pitch = P.pitch[l];
        C[l].lg_q = P.lg_q[l];
        C[l].narrow = P.narrow[l];
        C[l].gpitch = g.lv[l].pitch;
        C[l].pyr_off = g.lv[l].pyr_off;
        C[l].fstride = g.lv[l].pyr_frame_stride;
        C[l].x_rx = (int)sx;
        sx += 16;
        C[l].y_ry = (int)sy;
        sy += 16;
        if (l > 0) {
            C[l].x_xt = (int)sx;
            sx = align_up(sx + (size_t)P.pitch[l] * sizeof(short2), 16);
            C[l].y_yt = (int)sy;
            sy = align_up(sy + (size_t)P.maxh[l] * sizeof(short2), 16);
        }
    }
    A.sx = (int)sx;
    A.sy = (int)sy;
    A.off_x = (int)sizeof(C);
    A.off_y = A.off_x + (int)sx * P.ntx;
    blob.assign((size_t)A.off_y + sy * P.nty, 0);
    std::memcpy(blob.data(), C, sizeof(C));
    for (int ax = 0; ax < 2; ++ax) {
        const bool is_x = ax == 0;
        const int nt = is_x ? P.ntx : P.nty;
        const short4 *R = reg.data() + (is_x ? 0 : (size_t)NL * P.ntx);
        for (int t = 0; t < nt; ++t) {
            uint8_t *part = blob.data() + (is_x ? (size_t)A.off_x + sx * t : (size_t)A.off_y + sy * t);
            for (int l = 0; l < NL; ++l) {
                const short4 r = R[(size_t)l * nt + t];
                std::memcpy(part + (is_x ? C[l].x_rx : C[l].y_ry), &r, sizeof(r));
                if (l == 0) continue;
                const short4 rp = R[(size_t)(l - 1) * nt + t];
                const short2 *tb = tab + (is_x ? P.tabx[l] : P.taby[l]);
                const int dim = is_x ? g.lv[l].w : g.lv[l].h;
                short2 *out = reinterpret_cast<short2 *>(part + (is_x ? C[l].x_xt : C[l].y_yt));
                for (int i = 0; i <= r.y - r.x; ++i) {
                    short2 e{0, 0};  // columns past the level's width (dword padding): offset 0, weight 0
                    if (r.x + i < dim) {
                        e = tb[r.x + i];
                        e.x = (short)(e.x - rp.x);  // relative to the source region
                    }
                    out[i] = e;
                }
            }
        }
    }
    size_t off = sizeof(C);
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off = align_up(off + bytes, 16);
        return (int)o;
    };
    A.lds_x = take(sx);
    A.lds_y = take(sy);
    size_t buf[2] = {0, 0};
    for (int l = 0; l < NL; ++l) buf[l & 1] = std::max(buf[l & 1], (size_t)P.pitch[l] * P.maxh[l]);
    A.off_buf[0] = take(buf[0] + 16);  // + slack: the dword-read form fetches up to 12 bytes past a row's last tap
    A.off_buf[1] = take(buf[1] + 16);
    lds = off;
}
// the plan for the context's geometry
static int build_pyr_fuse(afv_ctx *c, const Geo &g, const short2 *tab) {
    std::vector<short4> reg;
    PyrFusePlan P;
    c->pf_ok = false;
    if (!plan_pyr_fuse(g, tab, c->tab_off_x, c->tab_off_y, c->pf_tw, c->pf_th, reg, P)) return AFV_OK;
    std::vector<uint8_t> blob;
    pack_pyr_fuse(g, tab, reg, P, blob, c->pf, c->pf_lds);
    if ((size_t)(sizeof(PfLevelC) * AFV_MAX_LEVELS + c->pf.sx + c->pf.sy) / 4 > 2 * 1024) return AFV_OK;  // the prologue copies <= 2 dwords per thread
    if (!afv_pyramid_fused_prepare(c->pf_lds)) return AFV_OK;
    if (blob.size() > c->pf_blob_cap) {
        if (c->d_pf_blob) (void)hipFree(c->d_pf_blob);
        c->d_pf_blob = nullptr;
        c->pf_blob_cap = 0;
        HIPCHK(c, hipMalloc(&c->d_pf_blob, blob.size()));
        c->pf_blob_cap = blob.size();
    }
    HIPCHK(c, hipMemcpy(c->d_pf_blob, blob.data(), blob.size(), hipMemcpyHostToDevice));
    c->pf.blob = c->d_pf_blob;
    c->pf_ok = true;
    return AFV_OK;
}

// host-only view of the plan and of the coefficient tables (no device needed): tests/test_host_logic.py replays the one-launch pyramid
// on the CPU from exactly these numbers and compares it with the level-by-level resize
extern "C" int afv_debug_pyramid_plan(const afv_orb_params *p, int width, int height, int tile_w, int tile_h, int16_t *regions, int regions_cap,
                                      int32_t *info, int16_t *tables, int tables_cap) {
    if (!p || !regions || !info) return AFV_EINVAL;
    Geo g;
    const int rc = afv_build_geometry(*p, width, height, 1, g);
    if (rc) return rc;
    size_t tox[AFV_MAX_LEVELS] = {}, toy[AFV_MAX_LEVELS] = {}, n = 0;
    for (int l = 1; l < g.nlevels; ++l) n += (size_t)g.lv[l].w + (size_t)g.lv[l].h;
    std::vector<short2> tab(std::max<size_t>(n, 1));
    size_t off = 0;
    for (int l = 1; l < g.nlevels; ++l) {
        tox[l] = off;
        resize_table(g.lv[l - 1].w, g.lv[l].w, tab.data() + off);
        off += (size_t)g.lv[l].w;
        toy[l] = off;
        resize_table(g.lv[l - 1].h, g.lv[l].h, tab.data() + off);
        off += (size_t)g.lv[l].h;
    }
    std::vector<short4> reg;
    PyrFusePlan A;
    if (!plan_pyr_fuse(g, tab.data(), tox, toy, tile_w, tile_h, reg, A)) return AFV_EUNSUPPORTED;
    std::vector<uint8_t> blob;
    PyrFuseArgs args;
    size_t lds = 0;
    pack_pyr_fuse(g, tab.data(), reg, A, blob, args, lds);
    if ((int)reg.size() * 4 > regions_cap || (tables && (int)n * 2 > tables_cap)) return AFV_ECAPACITY;
    std::memcpy(regions, reg.data(), reg.size() * sizeof(short4));
    if (tables) std::memcpy(tables, tab.data(), n * sizeof(short2));
    int k = 0;
    info[k++] = g.nlevels;
    info[k++] = A.ntx;
    info[k++] = A.nty;
    info[k++] = (int)lds;
    for (int l = 0; l < AFV_MAX_LEVELS; ++l) info[k++] = g.lv[l].w;
    for (int l = 0; l < AFV_MAX_LEVELS; ++l) info[k++] = g.lv[l].h;
    for (int l = 0; l < AFV_MAX_LEVELS; ++l) info[k++] = A.pitch[l];
    for (int l = 0; l < AFV_MAX_LEVELS; ++l) info[k++] = A.lg_q[l];
    for (int l = 0; l < AFV_MAX_LEVELS; ++l) info[k++] = A.tabx[l];
    for (int l = 0; l < AFV_MAX_LEVELS; ++l) info[k++] = A.taby[l];
    return AFV_OK;  // info: 4 + 6 * AFV_MAX_LEVELS ints
}

static int set_geometry(afv_ctx *c, int w, int h) {
    if (c->geo_valid && c->geo.width == w && c->geo.height == h) return AFV_OK;
    if (w > c->p.max_width || h > c->p.max_height) return AFV_EINVAL;
    Geo g;
    const int rc = afv_build_geometry(c->p, w, h, c->p.max_batch, g);
    if (rc) return rc;
    // allocation layout always follows the capacity geometry so buffers never move
    if (g.sel_per_frame > c->cap_geo.sel_per_frame) return AFV_EINVAL;  // wider aspect ratio than the capacity geometry
    for (int l = 0; l < g.nlevels; ++l) {
        if (g.lv[l].cand_cap > c->cap_geo.lv[l].cand_cap || g.lv[l].pyr_frame_stride > c->cap_geo.lv[l].pyr_frame_stride)
            return AFV_EINVAL;
        g.lv[l].pyr_off = c->cap_geo.lv[l].pyr_off;
        g.lv[l].pyr_frame_stride = c->cap_geo.lv[l].pyr_frame_stride;
        g.lv[l].cand_off = c->cap_geo.lv[l].cand_off;
        g.lv[l].cand_frame_stride = c->cap_geo.lv[l].cand_frame_stride;
    }
    std::vector<short2> tab(c->tab_elems);
    size_t off = 0;
    for (int l = 1; l < g.nlevels; ++l) {
        c->tab_off_x[l] = off;
        resize_table(g.lv[l - 1].w, g.lv[l].w, tab.data() + off);
        off += (size_t)g.lv[l].w;
        c->tab_off_y[l] = off;
        resize_table(g.lv[l - 1].h, g.lv[l].h, tab.data() + off);
        off += (size_t)g.lv[l].h;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(c->d_tab, tab.data(), off * sizeof(short2), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_geo, &g, sizeof(Geo), hipMemcpyHostToDevice));
    {   // the one-launch pyramid of the small-batch path
        const int rc_pf = build_pyr_fuse(c, g, tab.data());
        if (rc_pf) return rc_pf;
    }
    c->geo = g;
    c->geo_valid = true;
    return AFV_OK;
}

extern "C" int afv_max_keypoints_per_frame(const afv_ctx *c) {
    if (!c) return AFV_EINVAL;
    int s = 0;
    for (int l = 0; l < c->cap_geo.nlevels; ++l) s += std::max(c->cap_geo.lv[l].quota + 2, 4 * c->cap_geo.n_ini);
    return s;
}

extern "C" int afv_get_geometry(const afv_ctx *c, afv_geometry *g) {
    if (!c || !g) return AFV_EINVAL;
    const Geo &s = c->geo_valid ? c->geo : c->cap_geo;
    std::memset(g, 0, sizeof(*g));
    g->nlevels = s.nlevels;
    g->width = s.width;
    g->height = s.height;
    for (int l = 0; l < s.nlevels; ++l) {
        g->lw[l] = s.lv[l].w;
        g->lh[l] = s.lv[l].h;
        g->lscale[l] = s.lv[l].scale;
        g->quota[l] = s.lv[l].quota;
        g->cv_quota[l] = s.lv[l].cv_quota;
        g->cand_cap[l] = s.lv[l].cand_cap;
    }
    return AFV_OK;
}

// ---- the pipeline ----
// The small-batch ("latency") path: kernels shaped for one or a few frames (Tracking extracts ONE frame per call, Frame.cc:186) -
// the whole pyramid in one launch, ... - same results bit for bit.  afv_set_small_batch_path: 0 = never, 1 = batches of at most
// `small_max_frames` frames (default), 2 = always (parity tests).
// kernels of one contiguous frame range [f0, f0 + nf) on stream s
// clear_status: this range is the whole call, *d_status is cleared ahead of its kernels (by the one-launch pyramid when there is one)
// d_desc == nullptr: keypoints only (afv_orb_detect); pyramid_only: nothing behind the pyramid (afv_orb_compute describes given keypoints on it)
// pyramid_done: an earlier pyramid_only call on this stream has built the pyramid of these frames and cleared their candidate counts, and
// the caller has cleared d_hq_n[f0] (enqueue_extract, schedule 1): only the kernels behind the pyramid
static void enqueue_range(afv_ctx *c, const FrameSrc &src, int f0, int nf, afv_keypoint *d_kps, uint8_t *d_desc, int cap, int *d_n,
                          int *d_status, hipStream_t s, bool clear_status = false, const DescribeMirror *mirror = nullptr, bool pyramid_only = false,
                          bool pyramid_done = false) {
    const Geo &g = c->geo;
    {   // work lists are indexed with afv_udiv (exact below AFV_MAX_WORK items): longer ranges go out in pieces
        const int per = std::max(std::max(g.total_tiles, afv_describe_blocks_per_frame(&g)), 1);
        const int max_nf = std::max(1, (AFV_MAX_WORK - 8) / per);
        if (nf > max_nf) {
            if (clear_status && d_status) (void)hipMemsetAsync(d_status, 0, sizeof(int), s);
            for (int b = 0; b < nf; b += max_nf)
                enqueue_range(c, src, f0 + b, std::min(max_nf, nf - b), d_kps, d_desc, cap, d_n, d_status, s, false, mirror, pyramid_only, pyramid_done);
            return;
        }
    }
    int *cnt0 = c->d_cand_count + (size_t)f0 * AFV_MAX_LEVELS;
    if (g.nlevels < 2 && !pyramid_done) {  // no pyramid launch to carry the clears
        (void)hipMemsetAsync(cnt0, 0, (size_t)nf * AFV_MAX_LEVELS * sizeof(int), s);
        (void)hipMemsetAsync(c->d_hq_n + f0, 0, sizeof(int), s);
    }
    const bool small = small_batch_path(c, nf);
    if (clear_status && d_status && !(small && c->pf_ok)) (void)hipMemsetAsync(d_status, 0, sizeof(int), s);
    if (pyramid_done) {
    } else if (small && c->pf_ok) {
        StageTimer t_(c, AFV_STAGE_PYRAMID, s, nf);
        PyrFuseArgs A = c->pf;
        A.zero_counts = cnt0;
        A.n_zero = nf * AFV_MAX_LEVELS;
        A.zero_one = c->d_hq_n + f0;
        A.zero_two = clear_status ? d_status : nullptr;
        afv_launch_pyramid_fused(&src, c->d_pyr, &A, c->pf_lds, f0, nf, s);
    } else {
        StageTimer t_(c, AFV_STAGE_PYRAMID, s, nf);
        for (int l = 1; l < g.nlevels; ++l) {
            const LevelGeo &S = g.lv[l - 1], &D = g.lv[l];
            const uint8_t *sp = (l == 1) ? src.base : c->d_pyr + S.pyr_off;
            const int spitch = (l == 1) ? src.stride : S.pitch;
            const size_t sframe = (l == 1) ? src.frame_stride : S.pyr_frame_stride;
            afv_launch_resize(sp, S.w, S.h, spitch, sframe, c->d_pyr + D.pyr_off, D.w, D.h, D.pitch, D.pyr_frame_stride,
                              c->d_tab + c->tab_off_x[l], c->d_tab + c->tab_off_y[l], f0, nf, l == 1 ? cnt0 : nullptr, nf * AFV_MAX_LEVELS,
                              l == 1 ? c->d_hq_n + f0 : nullptr, s);
        }
    }
    if (pyramid_only) return;
    {
        StageTimer t_(c, AFV_STAGE_FAST_NMS, s, nf);
        afv_launch_fast_nms(c->d_geo, g.total_tiles, &src, c->d_pyr, c->d_cand_packed, c->d_cand_count, f0, nf, s);
    }
    {
        StageTimer t_(c, AFV_STAGE_HARRIS, s, nf);
        afv_launch_retain_harris(c->d_geo, g.nlevels, &src, c->d_pyr, c->d_cand_packed, c->d_cand_count, c->d_l1, c->d_l1_count,
                                 c->d_l1_resp, c->d_hq + (size_t)f0 * c->hq_per_frame, c->d_hq_n + f0, f0, nf, small ? 1 : 0, s);
    }
    {
        StageTimer t_(c, AFV_STAGE_SELECT, s, nf);
        afv_launch_select(c->d_geo, g.nlevels, c->d_l1, c->d_l1_resp, c->d_l1_count, c->d_kept_xy, c->d_kept_resp,
                          c->d_kept_node, c->d_sel, c->d_sel_count, c->select_M, f0, nf, (small && c->select_wide_ok) ? 1 : 0, s);
    }
    {
        StageTimer t_(c, AFV_STAGE_DESCRIBE, s, nf);
        afv_launch_describe(c->d_geo, afv_describe_blocks_per_frame(&g), &src, c->d_pyr, c->d_sel, c->d_sel_count, d_kps, d_desc, cap, d_n,
                            d_status, f0, nf, mirror, s);
    }
}

static int enqueue_extract(afv_ctx *c, const FrameSrc &src, int nframes, afv_keypoint *d_kps, uint8_t *d_desc, int cap,
                           int *d_n, int *d_status, hipStream_t s) {
    if (nframes >= c->split_min_frames) {
        if (d_status) HIPCHK(c, hipMemsetAsync(d_status, 0, sizeof(int), s));
        // Two streams.  What the split buys and what it does not (kernel traces, profiles/r09): two launches that share the chip run at
        // about half speed each, whatever they are - a FAST launch beside its twin, or beside the other stream's Harris / select launches,
        // which then wait for the workgroup slots FAST holds (a turnstile that let one FAST launch run at a time took its same-name
        // overlap from 1.58 to 0 ms per step and stretched k_harris from 0.27 to 0.74 ms: the step was 1.1 % slower).  The split wins where
        // a kernel alone leaves the chip part empty: the ramp and tail of every launch, the short launches of the small pyramid levels and
        // the latency-bound select / retain kernels.  It loses at every hand-off between the streams, 10 to 20 us of idle chip each.
        HIPCHK(c, hipEventRecord(c->ev_fork, s));
        HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
        // automatic: chunks of ~85 frames (measured optimum at 640x480: large enough to fill the chip, small enough that the
        // latency-bound kernels of one chunk run beside other kernels of the other stream), and an EVEN number of them: an odd
        // last chunk runs with nothing beside it (256 frames: 2 chunks 1.55 ms, 3 chunks 1.61; 384: 4 chunks 2.25, 5 chunks 2.33);
        // re-measured under schedule 1 (512 frames: 4 / 6 / 8 chunks 2.301 / 2.294 / 2.346 ms per step; 1024: 8 / 12 / 16 chunks
        // 4.511 / 4.536 / 4.617; 384: 2 / 4 / 6 chunks 1.747 / 1.741 / 1.767): the rule stays
        const int K = c->split_chunks ? c->split_chunks : std::min(64, 2 * std::max(1, (int)((float)nframes / 170.0f + 0.45f)));
        if (c->split_schedule == 0) {
            for (int k = 0; k < K; ++k) {  // chunk k on stream k % 2
                const int b = (int)((long)nframes * k / K), e = (int)((long)nframes * (k + 1) / K);
                if (e > b) enqueue_range(c, src, b, e - b, d_kps, d_desc, cap, d_n, d_status, (k & 1) ? c->stream2 : s);
            }
        } else {
            // Schedule 1: frames [0, h) on the caller's stream, [h, nframes) on the second, each as its share of the K chunks, and
            //  - the pyramid of a stream's whole range first, 7 launches instead of 7 per chunk (the launches of the small levels are
            //    mostly ramp and tail: 42 launches took 0.30 ms of a 512-frame step, the same levels of the whole batch take 0.24 alone);
            //  - the caller's stream carries `lead` frames more, so that it ends last: it runs straight on into whatever the caller has
            //    enqueued behind this call (bench.py: the pair matcher) instead of waiting one hand-off for the second stream, and the
            //    second stream's late start behind the fork is paid for.  28 frames of 640 x 480 (about 55 us of this pipeline; scaled by
            //    the pixel count), at most a tenth of the batch: measured optimum of the second stream's share at 64 .. 256 frames 0.45,
            //    at 512 frames 0.47 (0.49: +0.9 %, 0.45: +0.7 %).
            const int Ks = (K + 1) / 2, K2 = K / 2;
            const double px = std::max(1.0, (double)c->geo.width * (double)c->geo.height);
            const int lead = std::min(nframes / 10, std::max(1, (int)(28.0 * 640.0 * 480.0 / px + 0.5)));
            const int h = std::min(nframes, (int)(((long)nframes * Ks + K - 1) / K) + (lead + 1) / 2);
            enqueue_range(c, src, 0, h, d_kps, d_desc, cap, d_n, d_status, s, false, nullptr, true);
            HIPCHK(c, hipMemsetAsync(c->d_hq_n, 0, (size_t)h * sizeof(int), s));  // every chunk owns the counter of its first frame
            if (nframes > h) {
                enqueue_range(c, src, h, nframes - h, d_kps, d_desc, cap, d_n, d_status, c->stream2, false, nullptr, true);
                HIPCHK(c, hipMemsetAsync(c->d_hq_n + h, 0, (size_t)(nframes - h) * sizeof(int), c->stream2));
            }
            for (int k = 0; k < Ks; ++k) {  // host order: the streams' chunks in turn
                const int b = (int)((long)h * k / Ks), e = (int)((long)h * (k + 1) / Ks);
                if (e > b) enqueue_range(c, src, b, e - b, d_kps, d_desc, cap, d_n, d_status, s, false, nullptr, false, true);
                if (k >= K2) continue;
                const int b2 = h + (int)((long)(nframes - h) * k / K2), e2 = h + (int)((long)(nframes - h) * (k + 1) / K2);
                if (e2 > b2) enqueue_range(c, src, b2, e2 - b2, d_kps, d_desc, cap, d_n, d_status, c->stream2, false, nullptr, false, true);
            }
        }
        HIPCHK(c, hipEventRecord(c->ev_join, c->stream2));
        HIPCHK(c, hipStreamWaitEvent(s, c->ev_join, 0));
    } else {
        enqueue_range(c, src, 0, nframes, d_kps, d_desc, cap, d_n, d_status, s, true);
    }
    HIPCHK(c, hipGetLastError());
    c->last_src = src;
    c->last_nframes = nframes;
    return AFV_OK;
}

// ---- what the host entry points share ----
// Once an entry point has checked its arguments: the context's device, the geometry of this image size, and whether this call records
// stage events (every prof_every-th extraction; timed == false: none, whatever the call before left behind)
static int begin_call(afv_ctx *c, int width, int height, bool timed = true) {
    HIPCHK(c, hipSetDevice(c->device));
    const int rc = set_geometry(c, width, height);
    if (rc) return rc;
    c->prof = timed && c->prof_every && (c->prof_tick_extract++ % (unsigned)c->prof_every) == 0;
    return AFV_OK;
}

// the context's staging buffer as the kernels' source, laid out for THIS geometry: frames back to back when the row pitch allows it
static FrameSrc staged_src(const afv_ctx *c, int width, int height) {
    const size_t pitch = align_up((size_t)width, 64);
    return FrameSrc{c->d_frames, (int)pitch, align_up(pitch * (size_t)height, 256)};
}

// Frames [f0, f0 + nf) from the caller's memory to their slots of c->d_frames, on stream s.  pinned (the caller has probed them): DMA'd
// where they lie; else gathered into the pinned arena first, as tight rows at gather_off + f * width * height (the caller has sized the
// arena), and DMA'd from there.
// join (the batch pipeline): ONE linear transfer for the range when its staging slots lie back to back without padding and, for
// page-locked frames, the caller's images do too; otherwise a 2-D copy per frame.
// !join (the single-frame calls, nf == 1): a page-locked image takes the 2-D copy whatever its layout, the arena's copy is linear when
// the staging rows are tight - the forms those calls were measured with.
static int stage_images(afv_ctx *c, const uint8_t *const *frames, int f0, int nf, int width, int height, int stride_bytes, bool pinned,
                        size_t gather_off, bool join, hipStream_t s) {
    const FrameSrc src = staged_src(c, width, height);
    const size_t pitch = (size_t)src.stride, fstride = src.frame_stride, frame_bytes = (size_t)width * height;
    uint8_t *gathered = c->h_stage + gather_off;
    if (!pinned) {
        // one copy into the arena, one DMA: strips (CPU copy of strip k + 1 beside the DMA of strip k) lose more to the per-transfer
        // latency of the copy engine (~6 us each, serialised) than the overlap wins (measured on one 640 x 480 frame: 4 strips +16 us)
        for (int f = f0; f < f0 + nf; ++f) {
            uint8_t *dst = gathered + (size_t)f * frame_bytes;
            if ((size_t)stride_bytes == (size_t)width) {
                std::memcpy(dst, frames[f], frame_bytes);
            } else {
                for (int y = 0; y < height; ++y) std::memcpy(dst + (size_t)y * width, frames[f] + (size_t)y * stride_bytes, (size_t)width);
            }
        }
    }
    // linear: device rows without padding, and frames that follow each other without a gap on both sides
    bool linear = pitch == (size_t)width && (join ? fstride == frame_bytes : nf == 1);
    if (pinned) {
        linear = linear && join && (size_t)stride_bytes == (size_t)width;
        for (int f = f0 + 1; f < f0 + nf && linear; ++f) linear = frames[f] == frames[f - 1] + frame_bytes;
    }
    if (linear) {
        HIPCHK(c, hipMemcpyAsync(c->d_frames + (size_t)f0 * fstride, pinned ? frames[f0] : gathered + (size_t)f0 * frame_bytes, frame_bytes * (size_t)nf,
                                 hipMemcpyHostToDevice, s));
        return AFV_OK;
    }
    for (int f = f0; f < f0 + nf; ++f) {
        const uint8_t *sp = pinned ? frames[f] : gathered + (size_t)f * frame_bytes;
        HIPCHK(c, hipMemcpy2DAsync(c->d_frames + (size_t)f * fstride, pitch, sp, pinned ? (size_t)stride_bytes : (size_t)width, (size_t)width,
                                   (size_t)height, hipMemcpyHostToDevice, s));
    }
    return AFV_OK;
}

namespace {
// whatever path leaves an entry point, no DMA may still be in flight into the caller's buffers or the staging arena: drains the lanes
// named (read when it fires: the copy lane is created on first use) unless the call has waited for them itself and disarmed it
struct Quiesce {
    const hipStream_t *lanes[3];
    bool armed = true;
    ~Quiesce() {
        for (const hipStream_t *l : lanes)
            if (armed && l && *l) (void)hipStreamSynchronize(*l);
    }
};

// one frame's results from the arena to the caller (null: that array is not wanted, or was DMA'd in place): the count clamped to the
// caller's room, AFV_ECAPACITY when it did not fit
static int hand_over(int n, int cap, const uint8_t *h_kps, const uint8_t *h_desc, afv_keypoint *kps, uint8_t *desc32, int *n_out) {
    const int m = std::max(std::min(n, cap), 0);
    if (n_out) *n_out = m;
    if (kps) std::memcpy(kps, h_kps, (size_t)m * sizeof(afv_keypoint));
    if (desc32) std::memcpy(desc32, h_desc, (size_t)m * AFV_DESC_BYTES);
    return n > cap ? AFV_ECAPACITY : AFV_OK;
}

// AFV_TRACE_HOST=1: where the host spends a plugin call (averages over 100 calls on stderr) - a measurement aid, off by default.
// mark() ends a phase; report() ends the last one of a call that ran to its end
struct HostTrace {
    double ts[7] = {};
    int k = 0;
    static bool on() {
        static const bool v = std::getenv("AFV_TRACE_HOST") != nullptr;
        return v;
    }
    HostTrace() { mark(); }
    void mark() {
        if (on() && k < 7) ts[k++] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
    }
    void report() {
        if (!on()) return;
        mark();
        static thread_local double acc[6] = {};
        static thread_local int ncalls = 0;
        for (int i = 0; i < 6; ++i) acc[i] += ts[i + 1] - ts[i];
        if (++ncalls % 100 == 0) {
            fprintf(stderr, "afv_orb_extract (us, mean of 100): probes + arena %.1f | upload enqueue %.1f | kernel launches %.1f | download enqueue %.1f | wait %.1f | hand-over %.1f\n",
                    acc[0] / 100, acc[1] / 100, acc[2] / 100, acc[3] / 100, acc[4] / 100, acc[5] / 100);
            for (double &v : acc) v = 0;
        }
    }
};

}  // namespace

// ---- the entry points ----
extern "C" int afv_orb_extract_batch_device(afv_ctx *c, const uint8_t *d_frames, int nframes, int width, int height,
                                            int stride_bytes, size_t frame_stride_bytes, afv_keypoint *d_kps,
                                            uint8_t *d_desc32, int cap_per_frame, int32_t *d_n_out, int32_t *d_status_out,
                                            void *stream) {
    if (!c || !d_frames || !d_kps || !d_desc32 || !d_n_out) return AFV_EINVAL;
    if (nframes < 1 || nframes > c->p.max_batch || cap_per_frame < 1 || stride_bytes < width) return AFV_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_frames) & 3) || (stride_bytes & 3) || (frame_stride_bytes & 3)) return AFV_EINVAL;
    const int rc = begin_call(c, width, height);
    if (rc) return rc;
    FrameSrc src{d_frames, stride_bytes, frame_stride_bytes};
    return enqueue_extract(c, src, nframes, d_kps, d_desc32, cap_per_frame, d_n_out, d_status_out,
                           stream ? (hipStream_t)stream : c->stream);
}

static int ensure_events(afv_ctx *c, size_t n) {
    while (c->pipe_ev.size() < n) {
        hipEvent_t e = nullptr;
        HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->pipe_ev.push_back(e);
    }
    return AFV_OK;
}

// Host-buffer batch (the vocabulary-builder shape, createVocabulary.cpp:161-174), software-pipelined over chunks of frames:
//   copy lane     ... D2H(k-1), H2D(k+1), D2H(k), H2D(k+2) ...   (one stream: the two directions do not overlap each other)
//   compute       pyramid .. describe of chunk k (alternating over the context's two streams)
// Page-locked caller memory is DMA'd in place (frames in, keypoints / descriptors out); pageable memory goes through the
// context's pinned arena with one CPU memcpy each way.  Results are identical to the serial path (same kernels, same chunks).
extern "C" int afv_orb_extract_batch(afv_ctx *c, const uint8_t *const *frames, int nframes, int width, int height,
                                     int stride_bytes, afv_keypoint *kps, uint8_t *desc32, int cap_per_frame, int *n_out) {
    if (!c || !frames || !kps || !desc32 || !n_out) return AFV_EINVAL;
    if (nframes < 1 || nframes > c->p.max_batch || cap_per_frame < 1 || stride_bytes < width) return AFV_EINVAL;
    for (int f = 0; f < nframes; ++f)
        if (!frames[f]) return AFV_EINVAL;
    int rc = begin_call(c, width, height);
    if (rc) return rc;
    return guarded(c, [&]() -> int {
        Quiesce quiesce{{&c->stream, &c->stream2, &c->stream_copy}};
        const FrameSrc src = staged_src(c, width, height);
        const int CH = nframes >= 2 * c->pipe_chunk ? c->pipe_chunk : nframes;  // small batches: one chunk (plugin path: 1 frame)
        const int nchunks = (nframes + CH - 1) / CH;
        rc = ensure_events(c, (size_t)nchunks * 3);
        if (rc) return rc;
        // in-place DMA needs the WHOLE output arrays page-locked
        const bool out_direct = is_pinned_range(kps, (size_t)nframes * cap_per_frame * sizeof(afv_keypoint)) &&
                                is_pinned_range(desc32, (size_t)nframes * cap_per_frame * AFV_DESC_BYTES);
        const int ocap = std::min(cap_per_frame, c->stage_cap);
        // pinned arena: [pageable frames of the chunks in flight][n][kps][desc] (only what is not DMA'd in place)
        // all or nothing: frames are DMA'd in place only when the first and the last frame of EVERY chunk are page-locked (a probe per
        // frame would cost as much as the extraction of a small batch); a mix of pinned and pageable frames inside a chunk is not supported
        bool all_pinned_in = true;
        for (int f = 0; f < nframes && all_pinned_in; f += CH)
            all_pinned_in = is_pinned_host(frames[f]) && is_pinned_host(frames[std::min(f + CH, nframes) - 1] + (size_t)(height - 1) * stride_bytes + width - 1);
        HostImage arena{c};
        const size_t frame_bytes = (size_t)width * height;
        const size_t in_off = 0, in_bytes = all_pinned_in ? 0 : frame_bytes * (size_t)nframes;
        const size_t n_off = align_up(in_off + in_bytes, 64), n_bytes = (size_t)nframes * sizeof(int);
        const size_t k_off = align_up(n_off + n_bytes, 64), k_bytes = out_direct ? 0 : (size_t)nframes * c->stage_cap * sizeof(afv_keypoint);
        const size_t d_off = align_up(k_off + k_bytes, 64), d_bytes = out_direct ? 0 : (size_t)nframes * c->stage_cap * AFV_DESC_BYTES;
        arena.resize(d_off + d_bytes, false);
        uint8_t *hb = arena.data();
        // one chunk (the single-frame plugin path): everything on the context's stream, no cross-stream hand-offs
        hipStream_t s_copy = c->stream, s_back = c->stream;
        if (nchunks > 1) {
            if (!c->stream_copy) HIPCHK(c, hipStreamCreateWithFlags(&c->stream_copy, hipStreamNonBlocking));
            s_copy = s_back = c->stream_copy;
            HIPCHK(c, hipMemsetAsync(c->d_status, 0, sizeof(int), c->stream));
            HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
            HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
            HIPCHK(c, hipStreamWaitEvent(s_copy, c->ev_fork, 0));  // earlier work of this context that still reads d_frames
        }
        // H2D of chunk k (on the copy lane; the single-chunk case runs everything on the context's stream)
        auto upload = [&](int k) -> int {
            const int f0 = k * CH, nf = std::min(CH, nframes - f0);
            const int rc_up = stage_images(c, frames, f0, nf, width, height, stride_bytes, all_pinned_in, in_off, true, s_copy);
            if (rc_up) return rc_up;
            if (nchunks > 1) HIPCHK(c, hipEventRecord(c->pipe_ev[3 * k], s_copy));
            return AFV_OK;
        };
        // Both directions share ONE copy lane: concurrent H2D + D2H halves each direction on this platform (measured 56 GB/s one
        // way, 24 + 24 GB/s both ways), so the lane carries H2D(k+AHEAD) behind D2H(k): uploads stay AHEAD chunks ahead of the compute.
        const int AHEAD = std::max(c->pipe_ahead, 1);
        for (int k = 0; k < std::min(AHEAD, nchunks); ++k) {
            rc = upload(k);
            if (rc) return rc;
        }
        for (int k = 0; k < nchunks; ++k) {
            const int f0 = k * CH, nf = std::min(CH, nframes - f0);
            hipEvent_t e_in = c->pipe_ev[3 * k], e_done = c->pipe_ev[3 * k + 1], e_out = c->pipe_ev[3 * k + 2];
            // ---- compute ----
            hipStream_t cs = (k & 1) ? c->stream2 : c->stream;
            if (nchunks > 1) HIPCHK(c, hipStreamWaitEvent(cs, e_in, 0));
            enqueue_range(c, src, f0, nf, c->d_kps, c->d_desc, c->stage_cap, c->d_n, c->d_status, cs, nchunks == 1);
            // ---- D2H ----
            if (nchunks > 1) {
                HIPCHK(c, hipEventRecord(e_done, cs));
                HIPCHK(c, hipStreamWaitEvent(s_back, e_done, 0));
            }
            HIPCHK(c, hipMemcpyAsync(hb + n_off + (size_t)f0 * sizeof(int), c->d_n + f0, (size_t)nf * sizeof(int), hipMemcpyDeviceToHost, s_back));
            if (out_direct && cap_per_frame == c->stage_cap) {  // same row length on both sides: two plain DMA transfers
                HIPCHK(c, hipMemcpyAsync(kps + (size_t)f0 * cap_per_frame, c->d_kps + (size_t)f0 * c->stage_cap,
                                         (size_t)nf * c->stage_cap * sizeof(afv_keypoint), hipMemcpyDeviceToHost, s_back));
                HIPCHK(c, hipMemcpyAsync(desc32 + (size_t)f0 * cap_per_frame * AFV_DESC_BYTES, c->d_desc + (size_t)f0 * c->stage_cap * AFV_DESC_BYTES,
                                         (size_t)nf * c->stage_cap * AFV_DESC_BYTES, hipMemcpyDeviceToHost, s_back));
            } else if (out_direct) {
                HIPCHK(c, hipMemcpy2DAsync(kps + (size_t)f0 * cap_per_frame, (size_t)cap_per_frame * sizeof(afv_keypoint),
                                           c->d_kps + (size_t)f0 * c->stage_cap, (size_t)c->stage_cap * sizeof(afv_keypoint),
                                           (size_t)ocap * sizeof(afv_keypoint), (size_t)nf, hipMemcpyDeviceToHost, s_back));
                HIPCHK(c, hipMemcpy2DAsync(desc32 + (size_t)f0 * cap_per_frame * AFV_DESC_BYTES, (size_t)cap_per_frame * AFV_DESC_BYTES,
                                           c->d_desc + (size_t)f0 * c->stage_cap * AFV_DESC_BYTES, (size_t)c->stage_cap * AFV_DESC_BYTES,
                                           (size_t)ocap * AFV_DESC_BYTES, (size_t)nf, hipMemcpyDeviceToHost, s_back));
            } else {
                HIPCHK(c, hipMemcpyAsync(hb + k_off + (size_t)f0 * c->stage_cap * sizeof(afv_keypoint), c->d_kps + (size_t)f0 * c->stage_cap,
                                         (size_t)nf * c->stage_cap * sizeof(afv_keypoint), hipMemcpyDeviceToHost, s_back));
                HIPCHK(c, hipMemcpyAsync(hb + d_off + (size_t)f0 * c->stage_cap * AFV_DESC_BYTES, c->d_desc + (size_t)f0 * c->stage_cap * AFV_DESC_BYTES,
                                         (size_t)nf * c->stage_cap * AFV_DESC_BYTES, hipMemcpyDeviceToHost, s_back));
            }
            HIPCHK(c, hipEventRecord(e_out, s_back));
            if (k + AHEAD < nchunks) {
                rc = upload(k + AHEAD);
                if (rc) return rc;
            }
        }
        HIPCHK(c, hipGetLastError());
        c->last_src = src;
        c->last_nframes = nframes;
        // ---- hand the chunks over as they complete ----
        int result = AFV_OK;
        for (int k = 0; k < nchunks; ++k) {
            const int f0 = k * CH, nf = std::min(CH, nframes - f0);
            HIPCHK(c, hipEventSynchronize(c->pipe_ev[3 * k + 2]));
            const int *hn = reinterpret_cast<const int *>(hb + n_off);
            for (int f = f0; f < f0 + nf; ++f) {
                const int rc_f = hand_over(hn[f], cap_per_frame, hb + k_off + (size_t)f * c->stage_cap * sizeof(afv_keypoint),
                                           hb + d_off + (size_t)f * c->stage_cap * AFV_DESC_BYTES, out_direct ? nullptr : kps + (size_t)f * cap_per_frame,
                                           out_direct ? nullptr : desc32 + (size_t)f * cap_per_frame * AFV_DESC_BYTES, n_out + f);
                if (rc_f) result = rc_f;
            }
        }
        // the context's streams are idle again (the next call may overwrite d_frames)
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream2));
        return result;
    });
}

// The plugin call (FeatureExtractor::operator(), FeatureExtractor.cpp:111-129: ONE host image in, host vectors out) without the batch
// pipeline's bookkeeping: no events, no output probes, everything on the context's stream: upload, kernels, the frame's tail if there is
// one, wait, hand over.  A pageable image takes one copy into the pinned arena and one DMA from there, a page-locked one is DMA'd where
// it lies; the results come back without a copy engine (see below).
// `frame` (afv_frame_extract): the describe kernel also writes the frame's device arrays, and k_frame_grid (per-feature arrays + grid) follows
// on the stream before the host waits.
// `keypoints_only` (afv_orb_detect): the last kernel writes keypoints (position, angle, response) and no descriptors.
static int extract_one(afv_ctx *c, const uint8_t *gray, int width, int height, int stride_bytes, afv_keypoint *kps, uint8_t *desc32, int cap,
                       int *n_out, afv_frame *frame = nullptr, bool keypoints_only = false) {
    Quiesce quiesce{{&c->stream}};
    HostTrace trace;
    const FrameSrc src = staged_src(c, width, height);
    hipStream_t s = c->stream;
    const bool pinned_in = is_pinned_range(gray, (size_t)(height - 1) * stride_bytes + width);
    // results: the describe kernel writes counts, keypoints and descriptors STRAIGHT into the pinned arena (device-visible host memory:
    // 60 KB of posted writes over the link) - no copy engine between the last kernel and the host (that hop cost ~7 us)
    const size_t kps_off = 256, desc_off = kps_off + align_up((size_t)c->stage_cap * sizeof(afv_keypoint), 256);
    const size_t res_bytes = desc_off + (size_t)c->stage_cap * AFV_DESC_BYTES;
    HostImage arena{c};
    const size_t res_off = align_up(pinned_in ? 0 : (size_t)width * height, 256);
    arena.resize(res_off + res_bytes, false);
    uint8_t *hres = arena.data() + res_off;
    const bool zero_copy_out = c->stage_pinned;  // (a pageable arena only exists when pinning failed: results then take the copy engine)
    trace.mark();  // probes + arena
    const int rc_up = stage_images(c, &gray, 0, 1, width, height, stride_bytes, pinned_in, 0, false, s);
    if (rc_up) return rc_up;
    trace.mark();  // upload enqueue
    DescribeMirror mir{nullptr, nullptr, nullptr};
    if (frame) mir = DescribeMirror{frame->d_kps, frame->d_desc, frame->d_n};
    // (a frame smaller than the staging capacity: slots beyond frame->cap would be written past its arrays - afv_frame_create sizes frames
    // for the context's capacity, afv_frame_extract checks)
    if (zero_copy_out) {
        enqueue_range(c, src, 0, 1, reinterpret_cast<afv_keypoint *>(hres + kps_off), keypoints_only ? nullptr : hres + desc_off, c->stage_cap,
                      reinterpret_cast<int *>(hres), c->d_status, s, true, frame ? &mir : nullptr);
    } else {
        enqueue_range(c, src, 0, 1, c->d_kps, keypoints_only ? nullptr : c->d_desc, c->stage_cap, c->d_n, c->d_status, s, true, frame ? &mir : nullptr);
    }
    // a resident frame: the host vectors are complete when the describe kernel is (it writes them straight into the pinned arena);
    // k_frame_grid, which only feeds later device-side consumers on the same stream, runs on while the call returns
    bool wait_event = false;
    if (frame && zero_copy_out) {
        wait_event = hipEventRecord(c->ev_fork, s) == hipSuccess;
        if (!wait_event) (void)hipGetLastError();
    }
    if (frame) {
        const int rc_grid = afv_frame_after_extract(frame, s);  // (a failed launch must not leave has_grid set over the zeroed memset: ADVICE r5)
        if (rc_grid) return rc_grid;
        if (frame->p.keep_pyramid) {  // the levels stay with the frame: device copies behind the kernels, read by later work on this stream
            const int rc_pyr = afv_frame_keep_pyramid(frame, src, s);
            if (rc_pyr) return rc_pyr;
        }
    }
    HIPCHK(c, hipGetLastError());
    trace.mark();  // kernel launches
    if (!zero_copy_out) {
        HIPCHK(c, hipMemcpyAsync(hres, c->d_n, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(hres + kps_off, c->d_kps, (size_t)c->stage_cap * sizeof(afv_keypoint), hipMemcpyDeviceToHost, s));
        if (!keypoints_only) HIPCHK(c, hipMemcpyAsync(hres + desc_off, c->d_desc, (size_t)c->stage_cap * AFV_DESC_BYTES, hipMemcpyDeviceToHost, s));
    }
    c->last_src = src;
    c->last_nframes = 1;
    trace.mark();  // download enqueue
    if (wait_event) HIPCHK(c, hipEventSynchronize(c->ev_fork));
    else HIPCHK(c, hipStreamSynchronize(s));
    trace.mark();  // wait
    quiesce.armed = false;
    const int n = *reinterpret_cast<const int *>(hres);
    if (frame) frame->n = std::min(std::max(n, 0), frame->cap);
    const int result = hand_over(n, cap, hres + kps_off, hres + desc_off, kps, keypoints_only ? nullptr : desc32, n_out);
    trace.report();  // hand-over
    return result;
}

extern "C" int afv_orb_extract(afv_ctx *c, const uint8_t *gray, int width, int height, int stride_bytes, afv_keypoint *kps,
                               uint8_t *desc32, int cap, int *n_out) {
    if (!c || !gray || !kps || !desc32 || !n_out) return AFV_EINVAL;
    if (cap < 1 || stride_bytes < width) return AFV_EINVAL;
    const int rc = begin_call(c, width, height);
    if (rc) return rc;
    return guarded(c, [&]() -> int { return extract_one(c, gray, width, height, stride_bytes, kps, desc32, cap, n_out); });
}

// ---- the two halves of the plugin call as entry points of their own (FeatureExtractor.h:123-124, Feature_orb32.cpp:26-53) ----
// detectKeypoints + filterKeypoints (E1-E7): what afv_orb_extract returns as keypoints, before any descriptor is computed
extern "C" int afv_orb_detect(afv_ctx *c, const uint8_t *gray, int width, int height, int stride_bytes, afv_keypoint *kps, int cap, int *n_out) {
    if (!c || !gray || !kps || !n_out) return AFV_EINVAL;
    if (cap < 1 || stride_bytes < width) return AFV_EINVAL;
    const int rc = begin_call(c, width, height);
    if (rc) return rc;
    return guarded(c, [&]() -> int { return extract_one(c, gray, width, height, stride_bytes, kps, nullptr, cap, n_out, nullptr, true); });
}

// computeDescriptors = cv::ORB::compute at caller-given keypoints (E8-E10): for every keypoint the rBRIEF descriptor at
// cvRound(pt / scale(octave)) of its OWN octave and at its OWN angle, on the blurred level with the unblurred apron - the pyramid is
// rebuilt from the image as cv::ORB::compute rebuilds levels 0 .. max octave (here: all levels, in one launch).  Keypoints are taken as
// they are (orb.cpp runByImageBorder with edgeThreshold 0 removes nothing); a keypoint whose octave is not a level of this context or
// whose centre does not lie on its level image is refused (AFV_EINVAL), nothing is described then.
extern "C" int afv_orb_compute(afv_ctx *c, const uint8_t *gray, int width, int height, int stride_bytes, const afv_keypoint *kps, int n, uint8_t *desc32) {
    if (!c || !gray || n < 0 || (n > 0 && (!kps || !desc32)) || stride_bytes < width) return AFV_EINVAL;
    // no stage events: a profiled extract before this call must not leave the flag set for the pyramid launch below
    const int rc = begin_call(c, width, height, false);
    if (rc) return rc;
    const Geo &g = c->geo;
    for (int i = 0; i < n; ++i) {
        const afv_keypoint &k = kps[i];
        if (k.octave < 0 || k.octave >= g.nlevels) return AFV_EINVAL;
        const LevelGeo &L = g.lv[k.octave];
        const float cx = rintf(k.x * L.inv_scale), cy = rintf(k.y * L.inv_scale);
        if (!(cx >= 0.f && cx <= (float)L.w && cy >= 0.f && cy <= (float)L.h)) return AFV_EINVAL;  // (also refuses NaN)
    }
    if (n == 0) return AFV_OK;
    return guarded(c, [&]() -> int {
        Quiesce quiesce{{&c->stream}};
        hipStream_t s = c->stream;
        const FrameSrc src = staged_src(c, width, height);
        // arena: [image][keypoints][descriptors]; device side of the keypoints / descriptors: the matcher staging buffer
        const size_t k_off = align_up((size_t)width * height, 256), k_bytes = (size_t)n * sizeof(afv_keypoint);
        const size_t d_off = align_up(k_off + k_bytes, 256), d_bytes = (size_t)n * AFV_DESC_BYTES;
        HostImage arena{c};
        arena.resize(d_off + d_bytes, false);
        uint8_t *hb = arena.data();
        int rc2 = ensure_match_buffer(c, d_off + d_bytes);
        if (rc2) return rc2;
        // the image goes through the arena without a probe: the keypoints take that way anyhow
        rc2 = stage_images(c, &gray, 0, 1, width, height, stride_bytes, false, 0, false, s);
        if (rc2) return rc2;
        std::memcpy(hb + k_off, kps, k_bytes);
        HIPCHK(c, hipMemcpyAsync(c->d_match + k_off, hb + k_off, k_bytes, hipMemcpyHostToDevice, s));
        enqueue_range(c, src, 0, 1, nullptr, nullptr, 0, nullptr, nullptr, s, false, nullptr, true);
        afv_launch_describe_given(c->d_geo, &src, c->d_pyr, reinterpret_cast<const afv_keypoint *>(c->d_match + k_off), n, c->d_match + d_off, 0, s);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(hb + d_off, c->d_match + d_off, d_bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        std::memcpy(desc32, hb + d_off, d_bytes);
        c->last_src = src;
        c->last_nframes = 1;
        return AFV_OK;
    });
}

// afv_frame_extract (afv_frame.hip): the same call with a frame attached
int afv_extract_into_frame(afv_ctx *c, afv_frame *f, const uint8_t *gray, int width, int height, int stride_bytes, afv_keypoint *kps,
                           uint8_t *desc32, int cap, int *n_out) {
    const int rc = begin_call(c, width, height);
    if (rc) return rc;
    if (f->cap < c->stage_cap) return AFV_ECAPACITY;  // the describe kernel writes up to stage_cap slots of the mirror
    return guarded(c, [&]() -> int { return extract_one(c, gray, width, height, stride_bytes, kps, desc32, cap, n_out, f); });
}

// E12 (FeatureExtractor.cpp:132-172, settings FeatureExtractor.cpp:52-55)
float afv_size_of_octave(const afv_ctx *c, int octave) {
    const float scale_factor_orb = 1.2f;
    const float max_size0 = powf(scale_factor_orb, float(8 - 1.0));
    const float max_size = max_size0, min_size = 1.0f;
    const float s = powf(c->p.scale_factor, float(octave));  // GetKeypointSize Feature_orb32.cpp:59-61
    float norm = max_size;
    if (max_size > min_size) norm = 1.0f + (s - min_size) * (max_size0 - 1.0f) / (max_size - min_size);
    return norm;
}
extern "C" int afv_orb_size_sigma(const afv_ctx *c, const afv_keypoint *kps, int n, float *size, float *sigma2, float *inf) {
    if (!c || (n > 0 && (!kps || !size || !sigma2 || !inf)) || n < 0) return AFV_EINVAL;
    for (int i = 0; i < n; ++i) {
        const float norm = afv_size_of_octave(c, kps[i].octave);
        size[i] = norm;
        const float s2 = norm * norm;
        sigma2[i] = s2;
        inf[i] = 1.0f / s2;
    }
    return AFV_OK;
}

// ---- debug getters ----
static const uint8_t *level_ptr(const afv_ctx *c, int frame, int level, int *pitch) {
    const LevelGeo &L = c->geo.lv[level];
    if (level == 0) {
        *pitch = c->last_src.stride;
        return c->last_src.base + (size_t)frame * c->last_src.frame_stride;
    }
    *pitch = L.pitch;
    return c->d_pyr + L.pyr_off + (size_t)frame * L.pyr_frame_stride;
}

extern "C" int afv_debug_get_level(afv_ctx *c, int frame, int level, uint8_t *out) {
    if (!c || !out || !c->geo_valid || frame < 0 || frame >= c->last_nframes || level < 0 || level >= c->geo.nlevels) return AFV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    int pitch;
    const uint8_t *p = level_ptr(c, frame, level, &pitch);
    const LevelGeo &L = c->geo.lv[level];
    HIPCHK(c, hipMemcpy2D(out, (size_t)L.w, p, (size_t)pitch, (size_t)L.w, (size_t)L.h, hipMemcpyDeviceToHost));
    return AFV_OK;
}

extern "C" int afv_debug_get_candidates(afv_ctx *c, int frame, int level, uint32_t *packed, float *response, int cap, int *n_out) {
    if (!c || !packed || !response || !n_out || !c->geo_valid || frame < 0 || frame >= c->last_nframes || level < 0 ||
        level >= c->geo.nlevels)
        return AFV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    int n = 0;
    HIPCHK(c, hipMemcpy(&n, c->d_cand_count + frame * AFV_MAX_LEVELS + level, sizeof(int), hipMemcpyDeviceToHost));
    const LevelGeo &L = c->geo.lv[level];
    n = std::min(n, L.cand_cap);
    *n_out = n;
    const int m = std::min(n, cap);
    const size_t base = L.cand_off + (size_t)frame * L.cand_frame_stride;
    if (m > 0) {
        HIPCHK(c, hipMemcpy(packed, c->d_cand_packed + base, (size_t)m * 4, hipMemcpyDeviceToHost));
        // the Harris response exists for the candidates that survived retainBest on the score (the level's l1 list); 0 for the rest
        int n1 = 0;
        HIPCHK(c, hipMemcpy(&n1, c->d_l1_count + frame * AFV_MAX_LEVELS + level, sizeof(int), hipMemcpyDeviceToHost));
        n1 = std::min(std::max(n1, 0), L.cand_cap);
        std::vector<uint32_t> l1(std::max(n1, 1));
        std::vector<float> r1(std::max(n1, 1));
        if (n1 > 0) {
            HIPCHK(c, hipMemcpy(l1.data(), c->d_l1 + base, (size_t)n1 * 4, hipMemcpyDeviceToHost));
            HIPCHK(c, hipMemcpy(r1.data(), c->d_l1_resp + base, (size_t)n1 * 4, hipMemcpyDeviceToHost));
        }
        std::unordered_map<uint32_t, float> by_pos;
        by_pos.reserve((size_t)n1 * 2);
        for (int i = 0; i < n1; ++i) by_pos[l1[i] & 0x00ffffffu] = r1[i];
        for (int i = 0; i < m; ++i) {
            auto it = by_pos.find(packed[i] & 0x00ffffffu);
            response[i] = it == by_pos.end() ? 0.f : it->second;
        }
    }
    return n > cap ? AFV_ECAPACITY : AFV_OK;
}

extern "C" int afv_debug_get_selected(afv_ctx *c, int frame, int level, int32_t *x, int32_t *y, float *response, int cap, int *n_out) {
    if (!c || !x || !y || !response || !n_out || !c->geo_valid || frame < 0 || frame >= c->last_nframes || level < 0 ||
        level >= c->geo.nlevels)
        return AFV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    int n = 0;
    HIPCHK(c, hipMemcpy(&n, c->d_sel_count + frame * AFV_MAX_LEVELS + level, sizeof(int), hipMemcpyDeviceToHost));
    *n_out = n;
    const int m = std::min(n, cap);
    std::vector<SelPoint> tmp(std::max(m, 1));
    if (m > 0)
        HIPCHK(c, hipMemcpy(tmp.data(), c->d_sel + (size_t)frame * c->geo.sel_per_frame + c->geo.lv[level].sel_base,
                            (size_t)m * sizeof(SelPoint), hipMemcpyDeviceToHost));
    for (int i = 0; i < m; ++i) {
        x[i] = tmp[i].x;
        y[i] = tmp[i].y;
        response[i] = tmp[i].response;
    }
    return n > cap ? AFV_ECAPACITY : AFV_OK;
}

extern "C" int afv_debug_blur_level(afv_ctx *c, int frame, int level, uint8_t *out) {
    if (!c || !out || !c->geo_valid || frame < 0 || frame >= c->last_nframes || level < 0 || level >= c->geo.nlevels) return AFV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    int pitch;
    const uint8_t *p = level_ptr(c, frame, level, &pitch);
    const LevelGeo &L = c->geo.lv[level];
    uint8_t *d_out = nullptr;
    HIPCHK(c, hipMalloc(&d_out, (size_t)L.w * L.h));
    afv_launch_blur_level(p, L.w, L.h, pitch, d_out, c->stream);
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out, d_out, (size_t)L.w * L.h, hipMemcpyDeviceToHost);
    (void)hipFree(d_out);
    HIPCHK(c, e);
    return AFV_OK;
}
